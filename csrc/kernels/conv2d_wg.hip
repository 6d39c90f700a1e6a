// Weight and bias gradient of the client-grouped stride-1 2-D convolutions (the conv layers of lenet5, LeNet5_cifar,
// cnn_cifar10/100, the EMNIST CNNs and vgg11/16 — reference fedml_api/model/cv/{lenet5,cnn_cifar10,cnn,vgg}.py) on the
// matrix units, written where the gradient lives, and the weight-image pack that goes with it:
//     dW[g][co][ci][kh][kw] = sum over m = (b, oh, ow) of dY[g][m][co] X[g][b][oh + kh - pad][ow + kw - pad][ci]
//     dB[g][co]             = sum over m of dY[g][m][co]                                     (both fp32)
// X [G*B][H][W][cs] and dY [G*B][Ho][Wo][cout] are the channels-last bf16 tensors of HipConv2dFn; dW / dB are fp32
// blocks in the parameter layout [Cout][Cin][k][k] / [Cout] at a client stride (4-byte alignment only).  It replaces
// k_conv2d_any_wgrad (fp32 FMAs, one block per tap and 256-position chunk, partial slabs summed by the framework).
//
//  * 16x16x32 bf16 MFMA, fp32 accumulators; the contraction runs over the positions m, which are the ROW index of both
//    operands in memory, so 32-position tiles of dY and X go through LDS ([position][channel]) and both fragments are
//    read with the transposing ds_read_b64_tr_b16 (lg_tr_frag of linear_g.hip, with a row address per lane);
//  * grid (ci tile, co tile x kh, client): a block owns a 64 co x 64 ci tile (4 waves of 32 x 32) of the k taps of ONE
//    kernel row kh and holds all k accumulator sets (k x 4 f32x4 per wave: 80 VGPRs at k = 5).  It walks the whole
//    contraction M = B Ho Wo in 32-position steps: one block owns each output element, no split over positions, no
//    partial slabs, no atomics; the order of the additions is fixed by the shapes alone, so the same inputs give the
//    same bits;
//  * per step the dY tile (32 x 64) is stored to LDS once, and the X pixels that the k taps of the 32 positions read
//    are stored once, as a union: the positions of a step that share an output row (a "run") read Wo' + k - 1
//    consecutive pixels of input row oh + kh - pad, so run j takes that many union rows and tap kw of position p reads
//    union row u(p) + kw, u(p) = p + (k - 1) run(p).  A step may straddle output rows and samples (Wo = 2: 17 runs);
//    pixels outside the image, past M and union rows that no position of the step reads are stored as zeros.  Each X
//    and dY element is loaded from global memory once per (block, step); the next step's loads are issued into
//    registers before the current step's MFMAs and there are two LDS buffers, one barrier per step;
//  * narrow inputs (Cin <= 16: the first layers, Cin = 1 / 3 / 6): a 16-wide ci tile, the block's 4 waves each own
//    16 co x 16 ci x k taps.  A block still takes one kernel row, not all k x k taps: k times the blocks for the
//    few-client launches and one kernel body for both widths, at the price of staging dY k times per layer;
//  * channel loads are 16-B when the channel stride and count are multiples of 8 and the base is aligned, element
//    loads otherwise (c2_xfrag<false>'s rule);
//  * dB: the ci-tile-0 / kh-0 blocks sum the columns of their staged dY tiles in fp32, positions ascending;
//  * stores: a lane's k kw values of one (co, ci) are consecutive floats of the parameter layout (dword stores).
// Few clients with a long contraction (G = 8, 28 x 28 maps: M = 50 176 -> 1568 serial steps per block) stay
// latency-bound; a fixed-order split over positions is out of scope here, as in linear_g.hip.  The thin first layers
// (Cin <= 4) have one: conv2d_thin.hip's k_conv2d_thin_wgrad, which conv2d_hip.py routes them to.
// LDS: 2 x (32 x 72 + nu x (ci tile + 8)) bf16, nu = 32 + (k - 1) min(32, 1 + ceil(31 / Wo)) union rows; the launcher
// refuses shapes above 64 KiB (of k <= 7 only the 64-wide tile at k = 7 on 1-wide maps: 73 728 B; k = 6 there takes
// 64 512 B); conv2d_hip.py conv2d_wg_lds_bytes repeats this arithmetic.
// Resources (the flags of tools/build_ext.py, -O3 -fPIC -std=c++17 --offload-arch=gfx950, plus
// -Rpass-analysis=kernel-resource-usage; no scratch, no SGPR / VGPR spills in any instantiation;
// LDS is dynamic: 21 KiB for a 64-wide tile at k = 5 on maps of 31 or more columns, 28 KiB for vgg's k = 3, Wo = 2):
//     k               1    2    3    4    5    6    7
//     64-wide VGPRs  48   70   68   82   92   94  104    AGPRs  16   34   51   68   84  100  116
//     16-wide VGPRs  42   52   56   54   62   64   68    AGPRs   4   10   15   20   24   28   32
//     k_conv2d_pack_w: 10 VGPRs.
#include "common.h"

namespace nidt {

constexpr int kWgLdD = 72;  // LDS row stride of the dY tile in bf16 elements (linear_g.hip's padding)

struct C2WgTArgs {
  const uint16_t* x;   // [G*B][H][W][cs]
  const uint16_t* dy;  // [G*B][Ho][Wo][cout]
  float* dw;           // client 0's [cout][cin][k][k]
  float* db;           // client 0's [cout] or null
  int64_t lddw, lddb;  // client strides in elements
  int B, H, W, cin, cs, cout, pad, Ho, Wo, M, nu;
  int xvec, dvec;      // 16-B channel loads allowed for x / dy
};

// elements p[0 .. min(n, 8) - 1] and zeros after them; vec: n >= 8 and p is 16-B aligned whenever n > 0
__device__ __forceinline__ bf16x8 wg_ld8(const uint16_t* p, int n, bool vec) {
  bf16x8 v = {};
  if (n <= 0) return v;
  if (vec) return *reinterpret_cast<const bf16x8*>(p);
  uint16_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = j < n ? p[j] : (uint16_t)0;
  return __builtin_bit_cast(bf16x8, make_uint4(e[0] | (uint32_t)e[1] << 16, e[2] | (uint32_t)e[3] << 16,
                                               e[4] | (uint32_t)e[5] << 16, e[6] | (uint32_t)e[7] << 16));
}

// lg_tr_frag with the two LDS rows of this lane given by address: lane (fr, fq) hands in the rows of positions
// 8 fq + (fr >> 2) and + 4 at columns c + 4 (fr & 3) and receives column c + fr of positions 8 fq .. 8 fq + 7
__device__ __forceinline__ bf16x8 wg_tr_frag(const uint16_t* lo_row, const uint16_t* hi_row) {
  typedef short v4s __attribute__((ext_vector_type(4)));
  typedef short v8s __attribute__((ext_vector_type(8)));
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(lo_row));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(hi_row));
  const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

template <int K, bool NARROW>
__global__ __launch_bounds__(256) void k_conv2d_wg(C2WgTArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t wg_smem[];
  constexpr int CT = NARROW ? 16 : 64;           // ci tile
  constexpr int LDX = CT + 8;                    // union row stride (16-B multiple, rows off the same bank)
  constexpr int PPR = CT / 8;                    // 16-B pieces per union row
  constexpr int NPX = NARROW ? (K + 3) / 4 : K;  // pieces per thread at most: nu <= 32 K rows
  constexpr int NI = NARROW ? 1 : 2, NJ = NI;    // 16 x 16 tiles per wave along co, ci
  uint16_t* sD = wg_smem;                        // [2][32][kWgLdD]
  uint16_t* sX = wg_smem + 2 * 32 * kWgLdD;      // [2][nu][LDX]
  const int g = blockIdx.z, kh = blockIdx.y % K, co0 = (blockIdx.y / K) * 64, ci0 = blockIdx.x * CT;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int cob = NARROW ? 16 * wid : 32 * (wid & 1), cib = NARROW ? 0 : 32 * (wid >> 1);
  const int sr = tid >> 3, sc = (tid & 7) * 8;   // dY staging: position sr, channels sc .. sc + 7
  const int pa = 8 * fq + (fr >> 2), tc = 4 * (fr & 3);  // transposing reads: positions pa and pa + 4, columns tc ..
  const int Wu = a.Wo + K - 1;                   // union rows of a whole output row
  const int npieces = a.nu * PPR;
  const uint16_t* dg = a.dy + (int64_t)g * a.M * a.cout;
  const uint16_t* xg = a.x + (int64_t)g * a.B * a.H * a.W * a.cs;
  const bool bias_blk = a.db && blockIdx.x == 0 && kh == 0;  // block-uniform
  bf16x8 rd, rx[NPX];
  auto fetch = [&](int s) {
    const int m0 = 32 * s, m = m0 + sr;
    rd = wg_ld8(dg + (int64_t)(m < a.M ? m : 0) * a.cout + co0 + sc, m < a.M ? a.cout - co0 - sc : 0, a.dvec);
    // flattened (sample, output row) index and column of the step's first position; its run has L0 positions
    const int rl0 = m0 / a.Wo, ow0 = m0 - rl0 * a.Wo, L0 = a.Wo - ow0;
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
      const int pc = tid + 256 * i;
      rx[i] = bf16x8{};
      if (pc >= npieces) continue;
      const int r = pc / PPR, c = (pc % PPR) * 8;
      // union row r = pixel `off` of run j, whose first position is ps (column ows) of the step
      int j = 0, off = r, ps = 0, ows = ow0;
      if (r >= L0 + K - 1) {
        const int rr = r - (L0 + K - 1), q = rr / Wu;
        j = 1 + q; off = rr - q * Wu; ps = L0 + q * a.Wo; ows = 0;
      }
      const int rl = rl0 + j, n = rl / a.Ho, oh = rl - n * a.Ho;
      const int ih = oh + kh - a.pad, iw = ows + off - a.pad;
      // read by a position below 32 of the step, inside the batch, inside the image
      if (ps + max(0, off - (K - 1)) < 32 && rl < a.B * a.Ho && (unsigned)ih < (unsigned)a.H &&
          (unsigned)iw < (unsigned)a.W)
        rx[i] = wg_ld8(xg + (((int64_t)n * a.H + ih) * a.W + iw) * a.cs + ci0 + c, a.cin - ci0 - c, a.xvec);
    }
  };
  f32x4 acc[K][NI][NJ] = {};
  float dbs = 0.f;
  const int ns = (a.M + 31) / 32;
  fetch(0);
  for (int s = 0; s < ns; ++s) {
    uint16_t* bd = sD + (s & 1) * 32 * kWgLdD;  // its readers of step s - 2 are all past the barrier of step s - 1
    uint16_t* bx = sX + (s & 1) * a.nu * LDX;
    *reinterpret_cast<bf16x8*>(bd + sr * kWgLdD + sc) = rd;
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
      const int pc = tid + 256 * i;
      if (pc < npieces) *reinterpret_cast<bf16x8*>(bx + (pc / PPR) * LDX + (pc % PPR) * 8) = rx[i];
    }
    __syncthreads();
    if (s + 1 < ns) fetch(s + 1);
    const int m0 = 32 * s, rl0 = m0 / a.Wo;
    const int ua = pa + (K - 1) * ((m0 + pa) / a.Wo - rl0);          // u(pa)
    const int ub = pa + 4 + (K - 1) * ((m0 + pa + 4) / a.Wo - rl0);  // u(pa + 4)
    bf16x8 fa[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
      fa[i] = wg_tr_frag(bd + pa * kWgLdD + cob + 16 * i + tc, bd + (pa + 4) * kWgLdD + cob + 16 * i + tc);
#pragma unroll
    for (int kw = 0; kw < K; ++kw)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = cib + 16 * j + tc;
        const bf16x8 fb = wg_tr_frag(bx + (ua + kw) * LDX + c, bx + (ub + kw) * LDX + c);
#pragma unroll
        for (int i = 0; i < NI; ++i)
          acc[kw][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, acc[kw][i][j], 0, 0, 0);
      }
    if (bias_blk && tid < 64) {  // column co0 + tid of the staged dY rows, positions ascending (rows past M are zeros)
#pragma unroll 8
      for (int r = 0; r < 32; ++r) dbs += bf16_to_f32(bd[r * kWgLdD + tid]);
    }
  }
  // lane: co = co0 + cob + 16 i + 4 fq + r, ci = ci0 + cib + 16 j + fr, taps (kh, 0 .. K - 1): K consecutive floats
  float* dwg = a.dw + (int64_t)g * a.lddw;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + cob + 16 * i + 4 * fq + r;
      if (co >= a.cout) continue;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int ci = ci0 + cib + 16 * j + fr;
        if (ci >= a.cin) continue;
        float* p = dwg + (((int64_t)co * a.cin + ci) * K + kh) * K;
#pragma unroll
        for (int kw = 0; kw < K; ++kw) p[kw] = acc[kw][i][j][r];
      }
    }
  if (bias_blk && tid < 64 && co0 + tid < a.cout) a.db[(int64_t)g * a.lddb + co0 + tid] = dbs;
}

template <int K>
static void wg_launch(const C2WgTArgs& a, bool narrow, dim3 grid, size_t lds, hipStream_t s) {
  if (narrow)
    hipLaunchKernelGGL((k_conv2d_wg<K, true>), grid, dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((k_conv2d_wg<K, false>), grid, dim3(256), lds, s, a);
}

// db may be 0 (no bias gradient)
void conv2d_wg(uintptr_t x, uintptr_t dy, uintptr_t dw, int64_t lddw, uintptr_t db, int64_t lddb, int G, int B, int H,
               int W, int cin, int cs, int cout, int k, int pad, uintptr_t stream) {
  NIDT_REQUIRE(k >= 1 && k <= 7, "conv2d_wg: kernel size must be 1 .. 7");
  C2WgTArgs a;
  a.x = ptr<const uint16_t>(x); a.dy = ptr<const uint16_t>(dy); a.dw = ptr<float>(dw); a.db = ptr<float>(db);
  a.lddw = lddw; a.lddb = lddb;
  a.B = B; a.H = H; a.W = W; a.cin = cin; a.cs = cs; a.cout = cout; a.pad = pad;
  a.Ho = H + 2 * pad - k + 1;
  a.Wo = W + 2 * pad - k + 1;
  NIDT_REQUIRE(G > 0 && B > 0 && cin > 0 && cout > 0 && pad >= 0 && a.Ho > 0 && a.Wo > 0,
               "conv2d_wg: G, B, cin, cout and the output map must be positive");
  NIDT_REQUIRE(cs >= cin, "conv2d_wg: channel stride below cin");
  NIDT_REQUIRE((int64_t)B * a.Ho * a.Wo < (int64_t(1) << 31) - 64 && (int64_t)B * H * W < (int64_t(1) << 31),
               "conv2d_wg: positions per client must fit 31 bits");
  NIDT_REQUIRE(lddw >= (int64_t)cout * cin * k * k, "conv2d_wg: dw client stride below cout * cin * k * k");
  NIDT_REQUIRE(db == 0 || lddb >= cout, "conv2d_wg: db client stride below cout");
  a.M = B * a.Ho * a.Wo;
  const bool narrow = cin <= 16;
  const int nci = narrow ? 1 : (cin + 63) / 64, nco = (cout + 63) / 64;
  NIDT_REQUIRE(G <= 65535 && (int64_t)nco * k <= 65535, "conv2d_wg: grid too large");
  a.nu = 32 + (k - 1) * std::min(32, 1 + (31 + a.Wo - 1) / a.Wo);  // a step's runs: 1 + ceil(31 / Wo) at most
  const size_t lds = 2 * sizeof(uint16_t) * (32 * kWgLdD + (size_t)a.nu * ((narrow ? 16 : 64) + 8));
  NIDT_REQUIRE(lds <= 65536, "conv2d_wg: LDS tiles above 64 KiB (a 7 x 7 kernel with cin > 16 on a 1-wide output map)");
  a.xvec = cs % 8 == 0 && cin % 8 == 0 && x % 16 == 0;
  a.dvec = cout % 8 == 0 && dy % 16 == 0;
  const dim3 grid(nci, nco * k, G);
  hipStream_t s = as_stream(stream);
  switch (k) {
    case 1: wg_launch<1>(a, narrow, grid, lds, s); break;
    case 2: wg_launch<2>(a, narrow, grid, lds, s); break;
    case 3: wg_launch<3>(a, narrow, grid, lds, s); break;
    case 4: wg_launch<4>(a, narrow, grid, lds, s); break;
    case 5: wg_launch<5>(a, narrow, grid, lds, s); break;
    case 6: wg_launch<6>(a, narrow, grid, lds, s); break;
    default: wg_launch<7>(a, narrow, grid, lds, s); break;
  }
  NIDT_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// Both bf16 weight images of the clients' fp32 [cout][cin][k][k] blocks in one launch (RNE, zero padding written):
//   img  [g][ceil64(cout)][t][ceil8(cin)]  = W[g][co][ci][t]                     forward (pack_conv_w)
//   imgt [g][ceil64(cin)][t][ceil8(cout)]  = W[g][co][ci][k k - 1 - t]           data gradient (pack_conv_wt: flipped)
struct C2PackArgs {
  const float* w;
  uint16_t* img;
  uint16_t* imgt;  // or null
  int64_t ldw;
  int cout, cin, kt, cinp, coutp, n1, n2;  // n1 / n2: elements of one client's img / imgt (n2 = 0 without imgt)
};

__global__ __launch_bounds__(256) void k_conv2d_pack_w(C2PackArgs a) {
  const int g = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const float* wg = a.w + (int64_t)g * a.ldw;
  if (e < a.n1) {
    const int ci = e % a.cinp, q = e / a.cinp, t = q % a.kt, co = q / a.kt;
    const float v = co < a.cout && ci < a.cin ? wg[((int64_t)co * a.cin + ci) * a.kt + t] : 0.f;
    a.img[(int64_t)g * a.n1 + e] = f32_to_bf16(v);
  } else if (e - a.n1 < a.n2) {
    const int e2 = e - a.n1;
    const int co = e2 % a.coutp, q = e2 / a.coutp, t = q % a.kt, ci = q / a.kt;
    const float v = co < a.cout && ci < a.cin ? wg[((int64_t)co * a.cin + ci) * a.kt + (a.kt - 1 - t)] : 0.f;
    a.imgt[(int64_t)g * a.n2 + e2] = f32_to_bf16(v);
  }
}

// imgt may be 0 (evaluation: forward image only)
void conv2d_pack_w(uintptr_t w, int64_t ldw, uintptr_t img, uintptr_t imgt, int G, int cout, int cin, int k,
                   uintptr_t stream) {
  NIDT_REQUIRE(G > 0 && G <= 65535 && cout > 0 && cin > 0 && k >= 1, "conv2d_pack_w: G, cout, cin, k must be positive");
  NIDT_REQUIRE(ldw >= (int64_t)cout * cin * k * k, "conv2d_pack_w: weight client stride below cout * cin * k * k");
  C2PackArgs a;
  a.w = ptr<const float>(w); a.img = ptr<uint16_t>(img); a.imgt = ptr<uint16_t>(imgt); a.ldw = ldw;
  a.cout = cout; a.cin = cin; a.kt = k * k;
  a.cinp = (cin + 7) / 8 * 8;
  a.coutp = (cout + 7) / 8 * 8;
  const int64_t n1 = (int64_t)((cout + 63) / 64 * 64) * a.kt * a.cinp;
  const int64_t n2 = imgt ? (int64_t)((cin + 63) / 64 * 64) * a.kt * a.coutp : 0;
  NIDT_REQUIRE(n1 + n2 < (int64_t(1) << 31) - 256, "conv2d_pack_w: image size");
  a.n1 = (int)n1; a.n2 = (int)n2;
  hipLaunchKernelGGL(k_conv2d_pack_w, dim3((unsigned)((n1 + n2 + 255) / 256), G), dim3(256), 0, as_stream(stream), a);
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
