// Forward and stride-1 data gradient of the client-grouped 2-D convolutions (the conv layers of lenet5, cnn_cifar10/100,
// the EMNIST CNNs and vgg11/16 — reference fedml_api/model/cv/{lenet5,cnn_cifar10,cnn,vgg}.py) on an LDS-staged MFMA
// kernel, one body for both directions, on the channels-last bf16 tensors of HipConv2dFn:
//     Y [g][m][co] = bias[g][co] + sum_{kh,kw,ci} X [g][pix(m, kh, kw)][ci]             W[g][co][kh][kw][ci]   forward
//     dX[g][p][ci] =               sum_{kh,kw,co} dY[g][pix'(p, k-1-kh, k-1-kw)][co]    W[g][co][kh][kw][ci]   data gradient
// (the data gradient is a forward over dY with padding k - 1 - pad).  BOTH read the forward weight image
// [G][ceil64(Cout)][k k][ceil8(Cin)] of conv2d_pack_w; the flipped, transposed second image of k_conv2d_any_fwd's data
// gradient is never made.  It replaces k_conv2d_any_fwd (no LDS, every wave loading its own fragments from global
// memory) for the layers whose contraction channel count is a multiple of 8.  Measured (profiles/r13_conv2d_fd.txt,
// 100 clients x 16 images): 2.4x - 2.9x the old kernel forward (380 - 480 bf16 TF/s on the vgg11 layers) and
// 1.9x - 3.0x for the data gradient with its pack, from 64 contraction channels up.
//
//  * 16x16x32 bf16 MFMA, fp32 accumulators; block = 4 waves = 64 positions x 64 output channels, wave = 32 x 32; grid
//    (position tile, output-channel tile, client);
//  * the contraction walks (kernel row kh, 64-channel chunk, kw); a step is one tap of one chunk: 64 x 64 x 64;
//  * pixel union: per (kh, chunk) the pixels that the k taps of that kernel row read for the tile's 64 positions are
//    stored into LDS once: the positions of the tile that share an output row (a "run") read run length + k - 1
//    consecutive pixels of one input row, so tap kw of position p reads union row u(p) + kw,
//    u(p) = p + (k - 1) run(p) (conv2d_wg.hip's addressing on 64 positions).  A tile may straddle output rows and
//    samples (2 x 2 maps: 32 runs); pixels outside the image, positions past M = B Ho Wo, channels past the
//    contraction and union rows that no position reads are stored as zeros.  The B fragment (8 channels of one
//    position) is one 16-B LDS read;
//  * weight tiles: each tap's 64 co x 64 ci tile of the image goes through LDS as [co][ci], 128 contiguous bytes per
//    co row, two 16-B pieces per thread.  The forward (co = output channel, ci = contraction) reads its A fragment
//    with a plain 16-B LDS read; the data gradient (ci = output channel, co = contraction) reads the SAME tile with
//    the transposing ds_read_b64_tr_b16 (lg_tr_frag of linear_g.hip) and walks the taps flipped, k k - 1 - t.  Tile
//    columns at or beyond ceil8(Cin) do not exist in the image: they are not read and are stored as zeros;
//  * pipeline: the next step's weight pieces, and before the last tap of a kernel row the next union's pixels, are
//    loaded into registers before the current step's MFMAs; the weight tile has two LDS buffers and one barrier per
//    step.  Deviation from two buffers for everything: the union has ONE buffer and a second barrier in front of its
//    store (once per k steps).  Two union buffers put a 7 x 7 kernel on 3-wide maps (56 448 + 18 432 B) and a 3 x 3
//    kernel on 1-wide maps above 64 KiB and cost every shape a resident block per CU; one extra barrier per kernel row
//    and chunk is the cheaper price;
//  * a ragged last chunk of 32 channels or fewer issues half the MFMAs of a step;
//  * epilogue: fp32 bias (forward only), RNE to bf16, one 8-B store per 4 output channels when the channel count is
//    a multiple of 4 and the base is 8-B aligned, element stores otherwise;
//  * one block owns each output element and walks the whole contraction in an order fixed by the shapes alone: no
//    split, no atomics, the same inputs give the same bits.
// Served (the launcher raises on anything else and launches nothing): k <= 7, 0 <= pad (<= k - 1 for the data
// gradient), contraction channel count (cin forward, cout data gradient) and its stride multiples of 8, 16-B aligned
// operands, LDS within 64 KiB.  conv2d_hip.py conv2d_fd_served repeats the rule; conv2d_fd_ok adds the measured one
// (64 or more contraction channels: with 16 or 32 a step is half padding, profiles/r13_conv2d_fd.txt); the rest stays on
// k_conv2d_any_fwd.
// LDS (dynamic): 2 x 64 x 72 bf16 of weights + nu x 72 bf16 of union = 18 432 + 144 nu bytes,
// nu = 64 + (k - 1) min(64, 1 + ceil(63 / Wo)) with Wo the width of the map being written: 32 256 B for k = 5 on
// 10-wide maps (cnn_cifar10 conv2), 32 544 B for k = 3 on 4-wide, 37 152 B on 2-wide maps (vgg), 46 656 B for k = 7 on
// 3-wide maps; of k <= 7 only k = 6, 7 on 1-wide maps exceed 64 KiB (73 728 / 82 944 B).
// Resources (the flags of tools/build_ext.py, -O3 -fPIC -std=c++17 --offload-arch=gfx950, plus
// -Rpass-analysis=kernel-resource-usage; no scratch, no SGPR / VGPR spills in any instantiation):
//     k                 1    2    3    4    5    6    7
//     forward VGPRs     56   80   94  112  128  144  160     AGPRs 16 in all (the accumulators)
//     data grad VGPRs   56   76   96  110  128  144  160
// of which 10 k hold the 2 k union pieces in flight and their pixel indices (sized for 1-wide maps).
#include "common.h"

namespace nidt {

constexpr int kFdLd = 72;  // LDS row stride in bf16 elements (144 B: 16-B aligned, rows off the same bank)

struct C2FdArgs {
  const uint16_t* x;   // the tensor read:    [G*B][Hi][Wi][cs]  (X forward, dY data gradient)
  const uint16_t* w;   // forward weight image [G][coutp][k k][cinp]
  const float* bias;   // [G][O] or null
  uint16_t* y;         // the tensor written: [G*B][Ho][Wo][O]   (Y forward, dX data gradient)
  int64_t wrow, wcl;   // elements of one co row (k k cinp) and of one client's image
  int B, Hi, Wi, C, cs, O, pad, Ho, Wo, M, nu, cinp, nch;  // C contraction channels in nch chunks, O output channels
};

// lg_tr_frag of linear_g.hip on this file's stride: the contraction along the ROWS of an LDS tile [row][kFdLd]; lane
// (fr, fq) gets column c0 + fr, rows r0 + 8 fq .. + 7
__device__ __forceinline__ bf16x8 fd_tr_frag(const uint16_t* tile, int r0, int c0, int lane) {
  typedef short v4s __attribute__((ext_vector_type(4)));
  typedef short v8s __attribute__((ext_vector_type(8)));
  const int li = lane & 15;
  const uint16_t* p = tile + (r0 + 8 * (lane >> 4) + (li >> 2)) * kFdLd + c0 + 4 * (li & 3);
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p + 4 * kFdLd));
  const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

template <int K, bool DGRAD>
__global__ __launch_bounds__(256) void k_conv2d_fd(C2FdArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t fd_smem[];
  constexpr int KT = K * K;
  constexpr int NPX = 2 * K;                 // union pieces per thread at most: nu <= 64 K rows of 8 pieces
  uint16_t* sW = fd_smem;                    // [2][64][kFdLd]
  uint16_t* sU = fd_smem + 2 * 64 * kFdLd;   // [nu][kFdLd]
  const int g = blockIdx.z, o0 = blockIdx.y * 64, m0 = blockIdx.x * 64;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wp = wid & 1, wc = wid >> 1;     // wave: positions half wp, output channels half wc
  const int sr = tid >> 3, sc = (tid & 7) * 8;  // weight staging: tile rows sr and sr + 32, columns sc .. sc + 7
  const uint16_t* wg = a.w + (int64_t)g * a.wcl;
  const uint16_t* xg = a.x + (int64_t)g * a.B * a.Hi * a.Wi * a.cs;
  // flattened (sample, output row) index and column of the tile's first position; its run has L0 positions
  const int rl0 = m0 / a.Wo, ow0 = m0 - rl0 * a.Wo, L0 = a.Wo - ow0;
  const int Wu = a.Wo + K - 1;               // union rows of a whole output row
  const int npieces = a.nu * 8;
  int u[2];                                  // u(p) of this lane's two B columns (positions wp 32 + 16 j + fr)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = wp * 32 + 16 * j + fr;
    u[j] = p + (K - 1) * ((m0 + p) / a.Wo - rl0);
  }
  bf16x8 rw[2], rx[NPX];
  auto fetch_w = [&](int s) {  // step s = (kh nch + chunk) K + kw: its tap's 64 x 64 tile of the image
    const int kw = s % K, grp = s / K, ch = grp % a.nch, kh = grp / a.nch;
    const int t = DGRAD ? KT - 1 - (kh * K + kw) : kh * K + kw;
    const int r0 = DGRAD ? 64 * ch : o0, c = (DGRAD ? o0 : 64 * ch) + sc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      rw[i] = c < a.cinp ? *reinterpret_cast<const bf16x8*>(wg + (int64_t)(r0 + sr + 32 * i) * a.wrow + t * a.cinp + c)
                         : bf16x8{};
  };
  // the union piece i of this thread (row (tid + 256 i) / 8, channels (tid & 7) 8 .. + 7 of the chunk) does not move
  // with (kh, chunk): pxo = pixel index of its input column in the row kh = 0 reads, pxh = that row (oh - pad), or far
  // below zero for a piece that is always zeros
  int pxo[NPX], pxh[NPX];
#pragma unroll
  for (int i = 0; i < NPX; ++i) {
    const int r = (tid + 256 * i) >> 3;
    // union row r = pixel `off` of run j, whose first position is ps (column ows) of the tile
    int j = 0, off = r, ps = 0, ows = ow0;
    if (r >= L0 + K - 1) {
      const int rr = r - (L0 + K - 1), q = rr / Wu;
      j = 1 + q; off = rr - q * Wu; ps = L0 + q * a.Wo; ows = 0;
    }
    const int rl = rl0 + j, n = rl / a.Ho, oh = rl - n * a.Ho, iw = ows + off - a.pad;
    // a row of the union, read by a position below 64 of the tile, inside the batch, inside the image's columns
    const bool ok = r < a.nu && ps + max(0, off - (K - 1)) < 64 && rl < a.B * a.Ho && (unsigned)iw < (unsigned)a.Wi;
    pxh[i] = ok ? oh - a.pad : -(1 << 24);
    pxo[i] = ok ? (n * a.Hi + oh - a.pad) * a.Wi + iw : 0;
  }
  auto fetch_u = [&](int grp) {  // the union of (kh, chunk): zeros outside the image's rows and past the contraction
    const int ch = grp % a.nch, kh = grp / a.nch, c = 64 * ch + sc;
#pragma unroll
    for (int i = 0; i < NPX; ++i)
      rx[i] = (unsigned)(pxh[i] + kh) < (unsigned)a.Hi && c < a.C
                  ? *reinterpret_cast<const bf16x8*>(xg + ((int64_t)pxo[i] + kh * a.Wi) * a.cs + c)
                  : bf16x8{};
  };
  f32x4 acc[2][2] = {};
  const int ns = K * a.nch * K;
  fetch_w(0);
  fetch_u(0);
  for (int s = 0; s < ns; ++s) {
    const int kw = s % K, grp = s / K;
    if (kw == 0) {
      if (s) __syncthreads();  // the one union buffer: its readers of step s - 1 are done
#pragma unroll
      for (int i = 0; i < NPX; ++i) {
        const int pc = tid + 256 * i;
        if (pc < npieces) *reinterpret_cast<bf16x8*>(sU + (pc >> 3) * kFdLd + (pc & 7) * 8) = rx[i];
      }
    }
    uint16_t* sb = sW + (s & 1) * 64 * kFdLd;  // its readers of step s - 2 are all past the barrier of step s - 1
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<bf16x8*>(sb + (sr + 32 * i) * kFdLd + sc) = rw[i];
    __syncthreads();
    if (s + 1 < ns) {
      fetch_w(s + 1);
      if (kw == K - 1) fetch_u(grp + 1);
    }
    const int cl = a.C - 64 * (grp % a.nch);  // channels of this chunk (block-uniform)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (32 * kk >= cl) continue;
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int oc = wc * 32 + 16 * i;
        fa[i] = DGRAD ? fd_tr_frag(sb, 32 * kk, oc, lane)
                      : *reinterpret_cast<const bf16x8*>(sb + (oc + fr) * kFdLd + 32 * kk + 8 * fq);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(sU + (u[j] + kw) * kFdLd + 32 * kk + 8 * fq);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
  // lane: output channels o0 + wc 32 + 16 i + 4 fq + r (r = 0..3) of position m0 + wp 32 + 16 j + fr
  const float* bias = a.bias ? a.bias + (int64_t)g * a.O : nullptr;
  const bool pk = (a.O & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 7) == 0;  // rows of whole aligned 8-B pieces
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wp * 32 + 16 * j + fr;
    if (m >= a.M) continue;
    uint16_t* yp = a.y + ((int64_t)g * a.M + m) * a.O;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = o0 + wc * 32 + 16 * i + 4 * fq;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + (bias && c + r < a.O ? bias[c + r] : 0.f);
      if (pk && c + 3 < a.O) {
        *reinterpret_cast<uint2*>(yp + c) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (c + r < a.O) yp[c + r] = f32_to_bf16(v[r]);
      }
    }
  }
}

template <int K>
static void fd_launch(const C2FdArgs& a, bool dgrad, dim3 grid, size_t lds, hipStream_t s) {
  if (dgrad)
    hipLaunchKernelGGL((k_conv2d_fd<K, true>), grid, dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((k_conv2d_fd<K, false>), grid, dim3(256), lds, s, a);
}

// G, B, H, W, cin, cout, k, pad describe the forward layer in both directions.  dgrad = 0: x is X [G*B][H][W][cs],
// y is Y [G*B][Ho][Wo][cout].  dgrad = 1: x is dY [G*B][Ho][Wo][cs], y is dX [G*B][H][W][cin], bias must be 0.  cs is
// the channel stride of the tensor read; w is the forward image of conv2d_pack_w in both.
void conv2d_fd(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, int G, int B, int H, int W, int cin, int cs,
               int cout, int k, int pad, int dgrad, uintptr_t stream) {
  NIDT_REQUIRE(k >= 1 && k <= 7, "conv2d_fd: kernel size must be 1 .. 7");
  const int Ho = H + 2 * pad - k + 1, Wo = W + 2 * pad - k + 1;
  NIDT_REQUIRE(G > 0 && B > 0 && cin > 0 && cout > 0 && pad >= 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0,
               "conv2d_fd: G, B, cin, cout and both maps must be positive");
  NIDT_REQUIRE(!dgrad || (pad <= k - 1 && bias == 0), "conv2d_fd: the data gradient takes pad <= k - 1 and no bias");
  C2FdArgs a;
  a.x = ptr<const uint16_t>(x); a.w = ptr<const uint16_t>(w); a.bias = ptr<const float>(bias); a.y = ptr<uint16_t>(y);
  a.B = B; a.cs = cs;
  a.Hi = dgrad ? Ho : H; a.Wi = dgrad ? Wo : W; a.Ho = dgrad ? H : Ho; a.Wo = dgrad ? W : Wo;
  a.C = dgrad ? cout : cin; a.O = dgrad ? cin : cout; a.pad = dgrad ? k - 1 - pad : pad;
  NIDT_REQUIRE(a.C % 8 == 0 && cs % 8 == 0 && cs >= a.C,
               "conv2d_fd: the contraction channel count and its stride must be multiples of 8");
  NIDT_REQUIRE(x % 16 == 0 && w % 16 == 0, "conv2d_fd: x and the weight image must be 16-byte aligned");
  a.cinp = (cin + 7) / 8 * 8;
  a.wrow = (int64_t)k * k * a.cinp;
  a.wcl = (int64_t)((cout + 63) / 64 * 64) * a.wrow;
  NIDT_REQUIRE((int64_t)G * a.wcl < (int64_t(1) << 31), "conv2d_fd: weight image size");
  NIDT_REQUIRE((int64_t)B * a.Ho * a.Wo < (int64_t(1) << 31) - 64 && (int64_t)B * a.Hi * a.Wi < (int64_t(1) << 31),
               "conv2d_fd: positions per client must fit 31 bits");
  a.M = B * a.Ho * a.Wo;
  a.nch = (a.C + 63) / 64;
  a.nu = 64 + (k - 1) * std::min(64, 1 + (63 + a.Wo - 1) / a.Wo);  // a tile's runs: 1 + ceil(63 / Wo) at most
  const size_t lds = sizeof(uint16_t) * kFdLd * (2 * 64 + (size_t)a.nu);
  NIDT_REQUIRE(lds <= 65536, "conv2d_fd: LDS tiles above 64 KiB (a 6 x 6 or 7 x 7 kernel writing a 1-wide map)");
  const int nm = (a.M + 63) / 64, no = (a.O + 63) / 64;
  NIDT_REQUIRE(G <= 65535 && no <= 65535, "conv2d_fd: grid too large");
  const dim3 grid(nm, no, G);
  hipStream_t s = as_stream(stream);
  switch (k) {
    case 1: fd_launch<1>(a, dgrad, grid, lds, s); break;
    case 2: fd_launch<2>(a, dgrad, grid, lds, s); break;
    case 3: fd_launch<3>(a, dgrad, grid, lds, s); break;
    case 4: fd_launch<4>(a, dgrad, grid, lds, s); break;
    case 5: fd_launch<5>(a, dgrad, grid, lds, s); break;
    case 6: fd_launch<6>(a, dgrad, grid, lds, s); break;
    default: fd_launch<7>(a, dgrad, grid, lds, s); break;
  }
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
