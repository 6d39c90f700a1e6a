// Forward and weight / bias gradient of the client-grouped stride-1 2-D convolutions with THIN inputs: the first layer
// of every model of the 2-D zoo and of the EMNIST CNNs (Cin = 1 or 3: 1->20 k5, 3->6 k5, 3->64 k5, 3->64 k3, 1->32 k5,
// 1->32 k3 — reference fedml_api/model/cv/{lenet5,cnn_cifar10,cnn,vgg}.py).  conv2d_any.hip pads Cin to 8 (K = 200 for
// 75 real products at k = 5) and builds every fragment from 2-byte global loads; conv2d_wg.hip fills 3 of a 16-wide ci
// tile, stages dY k times and walks the whole contraction B Ho Wo in one block per (client, co tile, kernel row).
//
// The launcher's rule: Cin <= 4, k <= 7 and Kp = ceil32(Kd) <= 96, Kd = k k Cin; H, W, pad <= 4096; any Cout, any
// pad >= 0, H != W allowed.  Operands as in HipConv2dFn: x [G*B][H][W][cs] and y / dY [G*B][Ho][Wo][cout] bf16
// channels-last; weights, bias, dW, dB fp32 in the parameter layout [cout][cin][k][k] / [cout] at a client stride
// (4-byte alignment only).
//
//  * dense contraction, both kernels: kk = (kh k + kw) cin + c, walked as Kp / 32 16x16x32 bf16 MFMA k-steps (one
//    for vgg's k = 3, three for k = 5) instead of k k 8 / 32.  The im2col tile [positions][Kp] is built in LDS: a
//    thread owns one position of the tile and 8-element pieces of its row; each element's (kh, kw) and x offset
//    from the window's first pixel are computed once per block and stay in registers, a piece is 8 element loads (the
//    k cin values of one kernel row are consecutive in x when cs = cin) and one 16-B LDS store.  Pixels outside the
//    image, positions past the range and the tail Kd .. Kp - 1 are zeros;
//  * k_conv2d_thin_fwd, grid (tile group, co tile, client), 4 waves = 64 positions x 64 co, wave 32 x 32: no weight
//    image and no pack launch.  The block reads its 64 x Kd fp32 weight block in place, coalesced, rounds it with
//    f32_to_bf16 (conv2d_pack_w's helper: the same bits as the weight image) into LDS in kk order, and every wave
//    takes its weight fragments from there into registers ONCE; then the block walks `tpb` consecutive 64-position
//    tiles (tiles straddle rows and samples).  Per tile: the next tile's x elements are in registers before the
//    MFMAs, two LDS tile buffers, one barrier; both fragments are plain 16-B LDS reads (row stride Kp + 8: the 16
//    rows of a read fall on distinct banks); fp32 accumulators, fp32 bias, bf16 stores with conv2d_any_fwd's ragged
//    Cout handling;
//  * k_conv2d_thin_wgrad, grid (position split s, co tile, client): block s owns positions [s L, (s + 1) L), L a
//    multiple of 32, and accumulates a 64 x Kp fp32 tile (wave w: co 16 w .. + 15, all Kp columns: 2 Kp / 32
//    accumulators).  Per 32-position step the dY tile (32 x 64) and the im2col tile (32 x Kp) go through LDS and
//    both fragments are read with the transposing ds_read_b64_tr_b16 (the contraction index is the row index of both,
//    as in conv2d_wg.hip); the next step's loads sit in registers before the MFMAs, two LDS buffers, one barrier per
//    step.  dY is read once per layer.  The dB partial is the column sums of the staged dY tiles.  Each block writes
//    its partial (64 x Kp + 64 floats) to the scratch [client][co tile][s];
//  * k_conv2d_thin_finish sums the S partials in ascending s and writes dW [cout][cin][k][k] and dB at the client
//    stride.  No atomics; S (conv2d_thin_splits) is a function of G, B Ho Wo and Cout alone: about two blocks per CU
//    (512 blocks) with at least four steps per block, so the same inputs give the same bits.
// LDS (static): forward 3 x 64 x (Kp + 8) bf16 = 15 360 / 27 648 / 39 936 B at Kp = 32 / 64 / 96; weight gradient
// 2 x 32 x (72 + Kp + 8) bf16 = 14 336 / 18 432 / 22 528 B.
// Resources (the flags of tools/build_ext.py, -O3 -fPIC -std=c++17 --offload-arch=gfx950, plus
// -Rpass-analysis=kernel-resource-usage; no scratch, no SGPR / VGPR spills in any instantiation):
//     Kp                          32   64   96
//     k_conv2d_thin_fwd    VGPRs   68  108  146   AGPRs  16   20   20
//     k_conv2d_thin_wgrad  VGPRs   72   72  108   AGPRs   8   16   24
//     k_conv2d_thin_finish: 8 VGPRs.
#include "common.h"

namespace nidt {

constexpr int kThLdD = 72;       // LDS row stride of the dY tile in bf16 elements (conv2d_wg.hip's)
constexpr int kThMaxKp = 96;     // largest padded contraction served
constexpr int kThMaxHW = 4096;   // largest H, W, pad
constexpr int kThNever = 16384;  // kernel row of the elements kk >= Kd: never inside an image of kThMaxHW rows
constexpr int kThBlocks = 512;   // weight gradient: blocks aimed at (two per CU)
constexpr int kThMinSteps = 4;   // and the fewest 32-position steps a block is split down to

// Contraction element kk = (kh k + kw) cin + c: its x offset from the window's first pixel and kh << 16 | kw
__device__ __forceinline__ void th_tap(int kk, int Kd, int cin, int k, int W, int cs, int& off, int& hw) {
  const int t = kk / cin, c = kk - t * cin, kh = t / k, kw = t - kh * k;
  off = kk < Kd ? (kh * W + kw) * cs + c : 0;
  hw = kk < Kd ? (kh << 16 | kw) : (kThNever << 16);
}

// 8 im2col elements of the position whose window starts at pixel (ih0, iw0) = element `base` of the client's x
__device__ __forceinline__ bf16x8 th_gather(const uint16_t* xg, int64_t base, bool valid, int ih0, int iw0, int H,
                                            int W, const int (&off)[8], const int (&hw)[8]) {
  uint16_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ih = ih0 + (hw[j] >> 16), iw = iw0 + (hw[j] & 0xffff);
    e[j] = valid && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W ? xg[base + off[j]] : (uint16_t)0;
  }
  return __builtin_bit_cast(bf16x8, make_uint4(e[0] | (uint32_t)e[1] << 16, e[2] | (uint32_t)e[3] << 16,
                                               e[4] | (uint32_t)e[5] << 16, e[6] | (uint32_t)e[7] << 16));
}

// elements p[0 .. min(n, 8) - 1] and zeros after them; vec: n >= 8 and p is 16-B aligned whenever n > 0
__device__ __forceinline__ bf16x8 th_ld8(const uint16_t* p, int n, bool vec) {
  bf16x8 v = {};
  if (n <= 0) return v;
  if (vec) return *reinterpret_cast<const bf16x8*>(p);
  uint16_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = j < n ? p[j] : (uint16_t)0;
  return __builtin_bit_cast(bf16x8, make_uint4(e[0] | (uint32_t)e[1] << 16, e[2] | (uint32_t)e[3] << 16,
                                               e[4] | (uint32_t)e[5] << 16, e[6] | (uint32_t)e[7] << 16));
}

// conv2d_wg.hip's wg_tr_frag: lane (fr, fq) hands in the rows of positions 8 fq + (fr >> 2) and + 4 at columns
// c + 4 (fr & 3) and receives column c + fr of positions 8 fq .. 8 fq + 7
__device__ __forceinline__ bf16x8 th_tr_frag(const uint16_t* lo_row, const uint16_t* hi_row) {
  typedef short v4s __attribute__((ext_vector_type(4)));
  typedef short v8s __attribute__((ext_vector_type(8)));
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(lo_row));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(hi_row));
  const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// ------------------------------------------------------------------------------------------------ forward
struct ThFArgs {
  const uint16_t* x;  // [G*B][H][W][cs]
  const float* w;     // client 0's [cout][cin][k][k]
  const float* bias;  // client 0's [cout] or null
  uint16_t* y;        // [G*B][Ho][Wo][cout]
  int64_t ldw, ldb;   // client strides in elements
  int B, H, W, cin, cs, cout, k, pad, Ho, Wo, M, Kd;
  int ntiles, tpb;    // 64-position tiles per client, and per block
  int pk;             // 8-B stores of 4 channels allowed
};

template <int NK>
__global__ __launch_bounds__(256) void k_conv2d_thin_fwd(ThFArgs a) {
  constexpr int KP = 32 * NK, LDK = KP + 8;
  __shared__ __attribute__((aligned(16))) uint16_t sW[64 * LDK];
  __shared__ __attribute__((aligned(16))) uint16_t sA[2][64 * LDK];
  const int g = blockIdx.z, co0 = blockIdx.y * 64;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wp = wid & 1, wc = wid >> 1;  // wave: positions half wp, channels half wc
  // the block's weights: fp32 [co][c][t] read in place -> bf16 [co][t cin + c]; rows past cout and the tail are zeros
  for (int e = tid; e < 64 * LDK / 8; e += 256) reinterpret_cast<bf16x8*>(sW)[e] = bf16x8{};
  __syncthreads();
  {
    const float* wg = a.w + (int64_t)g * a.ldw + (int64_t)co0 * a.Kd;
    const int kt = a.k * a.k, ne = min(64, a.cout - co0) * a.Kd;
    for (int e = tid; e < ne; e += 256) {
      const int co = e / a.Kd, r = e - co * a.Kd, c = r / kt, t = r - c * kt;
      sW[co * LDK + t * a.cin + c] = f32_to_bf16(wg[e]);
    }
  }
  __syncthreads();
  bf16x8 fa[NK][2];
#pragma unroll
  for (int s = 0; s < NK; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      fa[s][i] = *reinterpret_cast<const bf16x8*>(sW + (wc * 32 + 16 * i + fr) * LDK + 32 * s + 8 * fq);
  // im2col: this thread builds pieces q + 4 i (elements 8 (q + 4 i) .. + 7) of row p of every tile
  const int p = tid >> 2, q = tid & 3;
  int off[NK][8], hw[NK][8];
#pragma unroll
  for (int i = 0; i < NK; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) th_tap(8 * (q + 4 * i) + j, a.Kd, a.cin, a.k, a.W, a.cs, off[i][j], hw[i][j]);
  const uint16_t* xg = a.x + (int64_t)g * a.B * a.H * a.W * a.cs;
  const int HoWo = a.Ho * a.Wo;
  bf16x8 rx[NK];
  auto fetch = [&](int tile) {
    const int m = 64 * tile + p;
    const bool mv = m < a.M;
    const int mm = mv ? m : 0;
    const int n = mm / HoWo, r = mm - n * HoWo, oh = r / a.Wo, ow = r - oh * a.Wo;
    const int ih0 = oh - a.pad, iw0 = ow - a.pad;
    const int64_t base = (((int64_t)n * a.H + ih0) * a.W + iw0) * a.cs;
#pragma unroll
    for (int i = 0; i < NK; ++i) rx[i] = th_gather(xg, base, mv, ih0, iw0, a.H, a.W, off[i], hw[i]);
  };
  const float* bias = a.bias ? a.bias + (int64_t)g * a.ldb : nullptr;
  const int t0 = blockIdx.x * a.tpb, t1 = min(t0 + a.tpb, a.ntiles);
  fetch(t0);
  for (int t = t0; t < t1; ++t) {
    uint16_t* buf = sA[(t - t0) & 1];  // its readers of tile t - 2 are all past the barrier of tile t - 1
#pragma unroll
    for (int i = 0; i < NK; ++i) *reinterpret_cast<bf16x8*>(buf + p * LDK + 8 * (q + 4 * i)) = rx[i];
    __syncthreads();
    if (t + 1 < t1) fetch(t + 1);
    f32x4 acc[2][2] = {};
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      bf16x8 fb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(buf + (wp * 32 + 16 * j + fr) * LDK + 32 * s + 8 * fq);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[s][i], fb[j], acc[i][j], 0, 0, 0);
    }
    // lane: output channels co0 + wc 32 + 16 i + 4 fq + r (r = 0..3) of position 64 t + wp 32 + 16 j + fr
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = 64 * t + wp * 32 + 16 * j + fr;
      if (m >= a.M) continue;
      uint16_t* yp = a.y + ((int64_t)g * a.M + m) * a.cout;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = co0 + wc * 32 + 16 * i + 4 * fq;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + (bias && c + r < a.cout ? bias[c + r] : 0.f);
        if (a.pk && c + 3 < a.cout) {
          *reinterpret_cast<uint2*>(yp + c) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (c + r < a.cout) yp[c + r] = f32_to_bf16(v[r]);
        }
      }
    }
  }
}

// The launcher's rule of both kernels (conv2d_hip.py conv2d_thin_served repeats it)
static int th_check(const char* who, int G, int B, int H, int W, int cin, int cs, int cout, int k, int pad) {
  const std::string n(who);
  NIDT_REQUIRE(k >= 1 && k <= 7 && cin >= 1 && cin <= 4, n + ": kernel size 1 .. 7 and 1 .. 4 input channels");
  const int kp = (k * k * cin + 31) / 32 * 32;
  NIDT_REQUIRE(kp <= kThMaxKp, n + ": k k cin rounded up to 32 must be at most 96");
  NIDT_REQUIRE(G > 0 && G <= 65535 && B > 0 && cout > 0 && cout <= 64 * 65535 && pad >= 0 && cs >= cin,
               n + ": G, B, cout must be positive, pad >= 0, channel stride >= cin");
  NIDT_REQUIRE(H > 0 && W > 0 && H <= kThMaxHW && W <= kThMaxHW && pad <= kThMaxHW, n + ": H, W, pad up to 4096");
  const int Ho = H + 2 * pad - k + 1, Wo = W + 2 * pad - k + 1;
  NIDT_REQUIRE(Ho > 0 && Wo > 0, n + ": empty output map");
  NIDT_REQUIRE((int64_t)B * Ho * Wo < (int64_t(1) << 31) - 64, n + ": positions per client must fit 31 bits");
  return kp;
}

// bias may be 0
void conv2d_thin_fwd(uintptr_t x, uintptr_t w, int64_t ldw, uintptr_t bias, int64_t ldb, uintptr_t y, int G, int B,
                     int H, int W, int cin, int cs, int cout, int k, int pad, uintptr_t stream) {
  const int kp = th_check("conv2d_thin_fwd", G, B, H, W, cin, cs, cout, k, pad);
  ThFArgs a;
  a.x = ptr<const uint16_t>(x); a.w = ptr<const float>(w); a.bias = ptr<const float>(bias); a.y = ptr<uint16_t>(y);
  a.ldw = ldw; a.ldb = ldb;
  a.B = B; a.H = H; a.W = W; a.cin = cin; a.cs = cs; a.cout = cout; a.k = k; a.pad = pad;
  a.Ho = H + 2 * pad - k + 1;
  a.Wo = W + 2 * pad - k + 1;
  a.M = B * a.Ho * a.Wo;
  a.Kd = k * k * cin;
  NIDT_REQUIRE(ldw >= (int64_t)cout * a.Kd, "conv2d_thin_fwd: weight client stride below cout * cin * k * k");
  NIDT_REQUIRE(bias == 0 || ldb >= cout, "conv2d_thin_fwd: bias client stride below cout");
  // about four blocks per CU, each walking tpb consecutive tiles with one weight block
  const int nco = (cout + 63) / 64;
  a.ntiles = (a.M + 63) / 64;
  const int nx = std::max(1, std::min(a.ntiles, (1024 + G * nco - 1) / (G * nco)));
  a.tpb = (a.ntiles + nx - 1) / nx;
  a.pk = cout % 4 == 0 && y % 8 == 0;
  const dim3 grid((a.ntiles + a.tpb - 1) / a.tpb, nco, G);
  hipStream_t s = as_stream(stream);
  switch (kp / 32) {
    case 1: hipLaunchKernelGGL(k_conv2d_thin_fwd<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_conv2d_thin_fwd<2>, grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(k_conv2d_thin_fwd<3>, grid, dim3(256), 0, s, a); break;
  }
  NIDT_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct ThWArgs {
  const uint16_t* x;   // [G*B][H][W][cs]
  const uint16_t* dy;  // [G*B][Ho][Wo][cout]
  float* part;         // [G][co tiles][S][64 Kp + 64]
  int B, H, W, cin, cs, cout, k, pad, Ho, Wo, M, Kd;
  int L, S;            // positions per block (a multiple of 32), blocks per (client, co tile)
  int dvec;            // 16-B channel loads allowed for dy
};

template <int NK>
__global__ __launch_bounds__(256) void k_conv2d_thin_wgrad(ThWArgs a) {
  constexpr int KP = 32 * NK, LDK = KP + 8;
  constexpr int NPX = (NK + 1) / 2;  // im2col pieces per thread: 4 NK pieces per position over 8 threads
  __shared__ __attribute__((aligned(16))) uint16_t sD[2][32 * kThLdD];
  __shared__ __attribute__((aligned(16))) uint16_t sX[2][32 * LDK];
  const int sp = blockIdx.x, co0 = blockIdx.y * 64, g = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int sr = tid >> 3, q = tid & 7, sc = q * 8;      // staging: position sr; dY channels sc .. + 7, pieces q + 8 i
  const int pa = 8 * fq + (fr >> 2), tc = 4 * (fr & 3);  // transposing reads: positions pa and pa + 4, columns tc ..
  int off[NPX][8], hw[NPX][8];
#pragma unroll
  for (int i = 0; i < NPX; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) th_tap(8 * (q + 8 * i) + j, a.Kd, a.cin, a.k, a.W, a.cs, off[i][j], hw[i][j]);
  const uint16_t* dg = a.dy + (int64_t)g * a.M * a.cout;
  const uint16_t* xg = a.x + (int64_t)g * a.B * a.H * a.W * a.cs;
  const int HoWo = a.Ho * a.Wo;
  const int m0 = sp * a.L, m1 = min(a.M, m0 + a.L);  // m0 < M: the launcher leaves no block an empty range
  bf16x8 rd, rx[NPX];
  auto fetch = [&](int s) {
    const int m = m0 + 32 * s + sr;
    const bool mv = m < m1;
    const int mm = mv ? m : 0;
    rd = th_ld8(dg + (int64_t)mm * a.cout + co0 + sc, mv ? a.cout - co0 - sc : 0, a.dvec);
    const int n = mm / HoWo, r = mm - n * HoWo, oh = r / a.Wo, ow = r - oh * a.Wo;
    const int ih0 = oh - a.pad, iw0 = ow - a.pad;
    const int64_t base = (((int64_t)n * a.H + ih0) * a.W + iw0) * a.cs;
#pragma unroll
    for (int i = 0; i < NPX; ++i) rx[i] = th_gather(xg, base, mv, ih0, iw0, a.H, a.W, off[i], hw[i]);
  };
  f32x4 acc[2 * NK] = {};
  float dbs = 0.f;
  const int ns = (m1 - m0 + 31) / 32;
  fetch(0);
  for (int s = 0; s < ns; ++s) {
    uint16_t* bd = sD[s & 1];  // its readers of step s - 2 are all past the barrier of step s - 1
    uint16_t* bx = sX[s & 1];
    *reinterpret_cast<bf16x8*>(bd + sr * kThLdD + sc) = rd;
#pragma unroll
    for (int i = 0; i < NPX; ++i)
      if (q + 8 * i < 4 * NK) *reinterpret_cast<bf16x8*>(bx + sr * LDK + 8 * (q + 8 * i)) = rx[i];
    __syncthreads();
    if (s + 1 < ns) fetch(s + 1);
    const bf16x8 fa = th_tr_frag(bd + pa * kThLdD + 16 * wid + tc, bd + (pa + 4) * kThLdD + 16 * wid + tc);
#pragma unroll
    for (int j = 0; j < 2 * NK; ++j) {
      const bf16x8 fb = th_tr_frag(bx + pa * LDK + 16 * j + tc, bx + (pa + 4) * LDK + 16 * j + tc);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[j], 0, 0, 0);
    }
    if (tid < 64) {  // column co0 + tid of the staged dY rows, positions ascending (rows past the range are zeros)
#pragma unroll 8
      for (int r = 0; r < 32; ++r) dbs += bf16_to_f32(bd[r * kThLdD + tid]);
    }
  }
  // lane: co = co0 + 16 wid + 4 fq + r, kk = 16 j + fr
  float* pt = a.part + (((int64_t)g * gridDim.y + blockIdx.y) * a.S + sp) * (64 * (KP + 1));
#pragma unroll
  for (int j = 0; j < 2 * NK; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) pt[(16 * wid + 4 * fq + r) * KP + 16 * j + fr] = acc[j][r];
  if (tid < 64) pt[64 * KP + tid] = dbs;
}

struct ThSArgs {
  const float* part;
  float* dw;           // client 0's [cout][cin][k][k]
  float* db;           // client 0's [cout] or null
  int64_t lddw, lddb;  // client strides in elements
  int cout, cin, kt, Kd, KP, S, nco;
};

// one thread per element of dW (in the order of the parameter layout) and of dB: the S partials in ascending s
__global__ __launch_bounds__(256) void k_conv2d_thin_finish(ThSArgs a) {
  const int g = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.cout * (a.Kd + 1)) return;
  const int co = e / (a.Kd + 1), r = e - co * (a.Kd + 1);
  const int64_t blk = 64 * (a.KP + 1);
  const float* p = a.part + ((int64_t)g * a.nco + (co >> 6)) * a.S * blk;
  int idx = 64 * a.KP + (co & 63);
  if (r < a.Kd) {
    const int c = r / a.kt, t = r - c * a.kt;
    idx = (co & 63) * a.KP + t * a.cin + c;
  }
  float v = 0.f;
  for (int s = 0; s < a.S; ++s) v += p[s * blk + idx];
  if (r < a.Kd)
    a.dw[(int64_t)g * a.lddw + (int64_t)co * a.Kd + r] = v;
  else if (a.db)
    a.db[(int64_t)g * a.lddb + co] = v;
}

// 32-position steps per client, and per block for `splits` blocks (0: by rule) per (client, co tile)
static void th_split(int G, int64_t M, int cout, int splits, int& S, int& lsteps) {
  const int nsteps = (int)((M + 31) / 32), gc = G * ((cout + 63) / 64);
  int want = splits > 0 ? splits : std::min((kThBlocks + gc - 1) / gc, nsteps / kThMinSteps);
  want = std::max(1, std::min(want, nsteps));
  lsteps = (nsteps + want - 1) / want;
  S = (nsteps + lsteps - 1) / lsteps;  // no block has an empty range
}

// The number of position splits of conv2d_thin_wgrad for a request `splits` (0: by rule): a function of the shapes
// alone.  The scratch takes G ceil(cout / 64) S (64 Kp + 64) floats, Kp = k k cin rounded up to 32.
int conv2d_thin_splits(int G, int B, int Ho, int Wo, int cout, int splits) {
  NIDT_REQUIRE(G > 0 && B > 0 && Ho > 0 && Wo > 0 && cout > 0 && splits >= 0, "conv2d_thin_splits: shape");
  int S, lsteps;
  th_split(G, (int64_t)B * Ho * Wo, cout, splits, S, lsteps);
  return S;
}

// db may be 0 (no bias gradient); part_floats: the capacity of the scratch
void conv2d_thin_wgrad(uintptr_t x, uintptr_t dy, uintptr_t dw, int64_t lddw, uintptr_t db, int64_t lddb,
                       uintptr_t part, int64_t part_floats, int splits, int G, int B, int H, int W, int cin, int cs,
                       int cout, int k, int pad, uintptr_t stream) {
  const int kp = th_check("conv2d_thin_wgrad", G, B, H, W, cin, cs, cout, k, pad);
  NIDT_REQUIRE(splits >= 0, "conv2d_thin_wgrad: splits must be 0 (by rule) or positive");
  ThWArgs a;
  a.x = ptr<const uint16_t>(x); a.dy = ptr<const uint16_t>(dy); a.part = ptr<float>(part);
  a.B = B; a.H = H; a.W = W; a.cin = cin; a.cs = cs; a.cout = cout; a.k = k; a.pad = pad;
  a.Ho = H + 2 * pad - k + 1;
  a.Wo = W + 2 * pad - k + 1;
  a.M = B * a.Ho * a.Wo;
  a.Kd = k * k * cin;
  NIDT_REQUIRE(lddw >= (int64_t)cout * a.Kd, "conv2d_thin_wgrad: dw client stride below cout * cin * k * k");
  NIDT_REQUIRE(db == 0 || lddb >= cout, "conv2d_thin_wgrad: db client stride below cout");
  int lsteps;
  th_split(G, a.M, cout, splits, a.S, lsteps);
  a.L = 32 * lsteps;
  const int nco = (cout + 63) / 64;
  NIDT_REQUIRE(part_floats >= (int64_t)G * nco * a.S * 64 * (kp + 1), "conv2d_thin_wgrad: scratch too small");
  a.dvec = cout % 8 == 0 && dy % 16 == 0;
  const dim3 grid(a.S, nco, G);
  hipStream_t s = as_stream(stream);
  switch (kp / 32) {
    case 1: hipLaunchKernelGGL(k_conv2d_thin_wgrad<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_conv2d_thin_wgrad<2>, grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(k_conv2d_thin_wgrad<3>, grid, dim3(256), 0, s, a); break;
  }
  NIDT_CHECK(hipGetLastError());
  ThSArgs f;
  f.part = a.part; f.dw = ptr<float>(dw); f.db = ptr<float>(db); f.lddw = lddw; f.lddb = lddb;
  f.cout = cout; f.cin = cin; f.kt = k * k; f.Kd = a.Kd; f.KP = kp; f.S = a.S; f.nco = nco;
  hipLaunchKernelGGL(k_conv2d_thin_finish, dim3((cout * (a.Kd + 1) + 255) / 256, G), dim3(256), 0, s, f);
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
