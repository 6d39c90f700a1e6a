// Forward and stride-1 data gradient of the client-grouped 2-D convolutions whose WEIGHTS are the dominant bytes (the
// deep 3 x 3 layers of vgg11/16 on 8 x 8 .. 2 x 2 maps — reference fedml_api/model/cv/vgg.py): conv2d_fd's semantics
// on the channels-last bf16 tensors of HipConv2dFn,
//     Y [g][m][co] = bias[g][co] + sum_{kh,kw,ci} X [g][pix(m, kh, kw)][ci]             W[g][co][ci][kh][kw]   forward
//     dX[g][p][ci] =               sum_{kh,kw,co} dY[g][pix'(p, k-1-kh, k-1-kw)][co]    W[g][co][ci][kh][kw]   data gradient
// (the data gradient is a forward over dY with padding k - 1 - pad), but W is the clients' fp32 parameter block
// [Cout][Cin][k][k], read where it lies in the parameter rows at a client stride: no bf16 weight image, no
// conv2d_pack_w launch, nothing saved for the backward.  conv2d_fd moves the weights three times (pack read, pack
// write, kernel read); this kernel reads them once per position tile.
//
//  * 16x16x32 bf16 MFMA, fp32 accumulators; block = 4 waves = TM positions x 64 output channels, grid (position tile,
//    output-channel tile, client).  TM = 64 (waves 2 x 2, each 32 x 32) or, from M = B Ho Wo = 256 positions up where
//    the slab fits, TM = 256 (wave w: positions 64 w .. + 63, all 64 channels, 4 x 4 fragments), so that a client's
//    16 images of a 4 x 4 map read the weights once;
//  * the contraction walks chunks of CK = 16 channels; per chunk ALL k k taps are in LDS, and an MFMA's four k-groups
//    are (tap, octet) pairs: k-group 4 s + fq = 2 tap + octet, ceil(2 k k / 4) MFMAs per fragment pair and chunk (5 for
//    k = 3, the last half zeros: lanes whose k-group is past 2 k k hand in zero fragments);
//  * weights streamed in memory order: forward, a block owns 64 output channels co and the chunk's 16 k k floats of
//    every co row are one contiguous run; data gradient, a block owns 64 output channels ci and every contraction row
//    co of the chunk holds the 64 k k floats of those ci as one contiguous run.  16 threads (forward) or a whole
//    wave (data gradient) sit side by side on a run and walk it in k k steps of 16 / 64 dwords, the block takes 16 / 4
//    runs per pass and 4 passes per chunk (4 k k dwords per thread and chunk); a dword's place in its run, and so its
//    tap, channel and LDS element, does not move with the chunk and is computed once: consecutive lanes read
//    consecutive dwords, 4-byte alignment is all that is asked.  Each value is rounded with f32_to_bf16 (the bits of
//    conv2d_pack_w's image) and scattered with a 2-byte LDS store to [tap][output channel][chunk channel]: row stride
//    24 elements (48 B: the 16 rows of a fragment read fall on all 64 banks), tap stride 64 x 24 + 8 (the k k taps of
//    consecutive dwords land 4 banks apart).  The data gradient stores tap t at k k - 1 - t: the flip is index
//    arithmetic, and every A fragment of both directions is one plain 16-B LDS read.  Rows past the output channels
//    and channels past the contraction are not read and stored as zeros;
//  * activations as whole padded samples: per chunk the block stores the zero-padded samples that its positions touch
//    as [sample][Hp][Wp][16], Hp = Ho + k - 1, row stride 24; tap (kh, kw) of position p is slab row
//    base(p) + kh Wp + kw, so one fill serves all k k taps (conv2d_fd refills its union per kernel row).  Tiles may
//    straddle samples; padding pixels, samples past B, channels past the contraction are zeros; positions past M read
//    row 0 and are not stored.  A slab piece (8 channels of one pixel) is one 16-B global load and LDS store, its
//    pixel index computed once per block;
//  * pipeline: the next chunk's weight dwords and slab pieces are loaded into registers before the current chunk's
//    MFMAs; one LDS buffer of each, two barriers per chunk (two weight buffers of a 3 x 3 kernel alone are 55 584 B);
//  * epilogue as in conv2d_fd: fp32 bias (forward only), RNE to bf16, one 8-B store per 4 output channels when the
//    channel count is a multiple of 4 and the base is 8-B aligned, element stores otherwise;
//  * one block owns each output element and walks the whole contraction in an order fixed by the shapes alone: no
//    split, no atomics, the same inputs give the same bits.  An accumulator adds 32 ceil(2 k k / 4) ceil(C / 16)
//    products, zeros included.
// Served (the launcher raises on anything else and launches nothing): k <= 3, 0 <= pad (<= k - 1 for the data
// gradient), contraction channel count (cin forward, cout data gradient) and its stride multiples of 8, 16-B aligned
// activations, ldw >= cout cin k k, and a slab of at most 768 rows (6 pieces per thread) within 64 KiB for TM = 64:
// ns Hp Wp rows, ns the most samples that a tile of TM positions touches (TM / P if P = Ho Wo divides TM, 1 if TM
// divides P, floor((TM + 2 P - 2) / P) otherwise, B at most).  conv2d_hip.py conv2d_ws_served repeats the rule;
// conv2d_ws_ok adds the measured one.
// LDS (dynamic): k k x 1544 bf16 of weights + 48 B per slab row = 27 792 B + 48 rows for k = 3: 40 080 B on 2 x 2 maps
// (TM = 64, 16 samples of 4 x 4), 55 440 B on 4 x 4 maps (TM = 256, 16 samples of 6 x 6), 46 992 B on 8 x 8 maps
// (TM = 256, 4 samples of 10 x 10), 43 344 B on 16 x 16 maps (TM = 256, one sample of 18 x 18); a 32 x 32 map
// (1156 rows) is not served.  k = 2: 12 352 B + 48 rows, k = 1: 3 088 B + 48 rows.
// Resources (the flags of tools/build_ext.py, -O3 -fPIC -std=c++17 --offload-arch=gfx950, plus
// -Rpass-analysis=kernel-resource-usage; no scratch, no SGPR / VGPR spills in any instantiation):
//     k                        1     2     3
//     forward   TM = 64        88   106   148   VGPRs     AGPRs 16 (TM = 64), 64 (TM = 256): the accumulators
//     forward   TM = 256      106   120   170
//     data grad TM = 64        80    98   136
//     data grad TM = 256       98   112   154
// of which 4 k k hold the weight dwords and 24 the slab pieces in flight.
// Measured (profiles/r16_conv2d_ws.txt, vgg's 3 x 3 layers, 100 clients x 16 images): forward 1.3x - 4.4x of
// conv2d_pack_w + conv2d_fd from 128 input channels up, HipConv2dFn forward + backward 1.1x - 1.9x, the vgg11 train
// step 0.73 and its evaluation 0.40 of the packed path.
#include "common.h"

namespace nidt {

constexpr int kWsCK = 16;                  // contraction channels per chunk
constexpr int kWsLd = 24;                  // LDS row stride in bf16 elements (48 B) of both tiles
constexpr int kWsTap = 64 * kWsLd + 8;     // LDS elements of one tap's [64][kWsLd] weight tile and its bank offset
constexpr int kWsNpx = 6;                  // slab pieces per thread at most
constexpr int kWsMaxRows = 128 * kWsNpx;   // slab rows at most (two 16-B pieces per row, 256 threads)

struct C2WsArgs {
  const uint16_t* x;   // the tensor read:    [G*B][Hi][Wi][cs]  (X forward, dY data gradient)
  const float* w;      // client 0's [cout][cin][k][k]
  const float* bias;   // client 0's [O] or null
  uint16_t* y;         // the tensor written: [G*B][Ho][Wo][O]   (Y forward, dX data gradient)
  int64_t ldw, ldb;    // client strides in elements
  int B, Hi, Wi, C, cs, O, pad, Ho, Wo, M, cin, nch;  // C contraction channels in nch chunks, O output channels
  int Hp, Wp, nrows;   // the padded sample and the slab rows of a tile
};

template <int K, bool DGRAD, int TM>
__global__ __launch_bounds__(256) void k_conv2d_ws(C2WsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ws_smem[];
  constexpr int KT = K * K;
  constexpr int NS = (2 * KT + 3) / 4;              // MFMAs per fragment pair and chunk
  constexpr int LW = DGRAD ? 64 : 16;               // threads side by side on one contiguous run of LW KT floats
  constexpr int RS = 256 / LW;                      // runs per pass of the block; 4 passes cover the chunk
  constexpr int NWD = 4 * KT;                       // weight dwords per thread and chunk
  constexpr int NF = TM == 64 ? 2 : 4;              // fragments per wave along positions and along channels
  uint16_t* sW = ws_smem;                           // [KT][kWsTap]: tap, output channel, chunk channel
  uint16_t* sX = ws_smem + KT * kWsTap;             // [nrows][kWsLd]
  const int g = blockIdx.z, o0 = blockIdx.y * 64, m0 = blockIdx.x * TM;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int pb = TM == 64 ? (wid & 1) * 32 : wid * 64;  // the wave's first position and output channel of the tile
  const int ob = TM == 64 ? (wid >> 1) * 32 : 0;
  const float* wg = a.w + (int64_t)g * a.ldw;
  const uint16_t* xg = a.x + (int64_t)g * a.B * a.Hi * a.Wi * a.cs;
  const int P = a.Ho * a.Wo, n0 = m0 / P, HpWp = a.Hp * a.Wp;
  int base[NF];  // LDS element of slab row base(p) of this lane's B columns (positions pb + 16 j + fr)
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int p = m0 + pb + 16 * j + fr;
    const int n = p / P, r = p - n * P, oh = r / a.Wo, ow = r - oh * a.Wo;
    base[j] = p < a.M ? (((n - n0) * a.Hp + oh) * a.Wp + ow) * kWsLd : 0;
  }
  int xo[NS], wo[NS];  // k-group 4 s + fq = (tap, octet): its offset in the slab and in the weight tiles
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int kg = 4 * s + fq, t = min(kg >> 1, KT - 1), oc8 = 8 * (kg & 1);
    xo[s] = ((t / K) * a.Wp + t % K) * kWsLd + oc8;
    wo[s] = t * kWsTap + (ob + fr) * kWsLd + oc8;
  }
  // slab piece i of this thread (row (tid + 256 i) / 2, channels 8 (tid & 1) .. + 7 of the chunk) does not move with
  // the chunk: px = its pixel index in the client's tensor, or -1 for a piece that is always zeros
  int px[kWsNpx];
#pragma unroll
  for (int i = 0; i < kWsNpx; ++i) {
    const int row = (tid + 256 * i) >> 1;
    const int nl = row / HpWp, rr = row - nl * HpWp, hp = rr / a.Wp, wq = rr - hp * a.Wp;
    const int n = n0 + nl, ih = hp - a.pad, iw = wq - a.pad;
    const bool ok = row < a.nrows && n < a.B && (unsigned)ih < (unsigned)a.Hi && (unsigned)iw < (unsigned)a.Wi;
    px[i] = ok ? (n * a.Hi + ih) * a.Wi + iw : -1;
  }
  // weight dword (rb, ei) of this thread: float wl + LW ei of run rb RS + wr.  Its place in the run does not move with
  // the chunk: wq = its channel of the run (forward: chunk channel, data gradient: output channel), wlds = its LDS
  // element for rb = 0
  const int wl = tid % LW, wr = tid / LW;
  int wq[KT], wlds[KT];
#pragma unroll
  for (int ei = 0; ei < KT; ++ei) {
    const int e = wl + LW * ei, q = e / KT, t = e - q * KT;
    wq[ei] = q;
    wlds[ei] = DGRAD ? (KT - 1 - t) * kWsTap + q * kWsLd + wr : t * kWsTap + wr * kWsLd + q;
  }
  float rw[NWD];
  bf16x8 rx[kWsNpx];
  auto fetch = [&](int ch) {  // chunk ch: its weight dwords in memory order and its slab pieces
    const int c0 = kWsCK * ch;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      const int row = rb * RS + wr;
      const bool rok = DGRAD ? c0 + row < a.C : o0 + row < a.O;
      const float* p = wg + (DGRAD ? (int64_t)(c0 + row) * a.cin + o0 : (int64_t)(o0 + row) * a.cin + c0) * KT + wl;
#pragma unroll
      for (int ei = 0; ei < KT; ++ei)
        rw[rb * KT + ei] = rok && (DGRAD ? o0 + wq[ei] < a.O : c0 + wq[ei] < a.C) ? p[LW * ei] : 0.f;
    }
    const int c = c0 + 8 * (tid & 1);
#pragma unroll
    for (int i = 0; i < kWsNpx; ++i)
      rx[i] = px[i] >= 0 && c < a.C ? *reinterpret_cast<const bf16x8*>(xg + (int64_t)px[i] * a.cs + c) : bf16x8{};
  };
  f32x4 acc[NF][NF] = {};
  fetch(0);
  for (int ch = 0; ch < a.nch; ++ch) {
    if (ch) __syncthreads();  // one buffer of each: the readers of chunk ch - 1 are done
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int ei = 0; ei < KT; ++ei) sW[wlds[ei] + rb * RS * (DGRAD ? 1 : kWsLd)] = f32_to_bf16(rw[rb * KT + ei]);
#pragma unroll
    for (int i = 0; i < kWsNpx; ++i) {
      const int pc = tid + 256 * i;
      if (pc < 2 * a.nrows) *reinterpret_cast<bf16x8*>(sX + (pc >> 1) * kWsLd + 8 * (pc & 1)) = rx[i];
    }
    __syncthreads();
    if (ch + 1 < a.nch) fetch(ch + 1);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bool kv = 4 * s + 3 < 2 * KT || 4 * s + fq < 2 * KT;  // k-groups past the taps are zeros on both sides
      bf16x8 fa[NF], fb[NF];
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        fa[i] = *reinterpret_cast<const bf16x8*>(sW + wo[s] + 16 * i * kWsLd);
        if (!kv) fa[i] = bf16x8{};
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        fb[j] = *reinterpret_cast<const bf16x8*>(sX + base[j] + xo[s]);
        if (!kv) fb[j] = bf16x8{};
      }
#pragma unroll
      for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
  // lane: output channels o0 + ob + 16 i + 4 fq + r (r = 0..3) of position m0 + pb + 16 j + fr
  const float* bias = a.bias ? a.bias + (int64_t)g * a.ldb : nullptr;
  const bool pk = (a.O & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 7) == 0;  // rows of whole aligned 8-B pieces
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int m = m0 + pb + 16 * j + fr;
    if (m >= a.M) continue;
    uint16_t* yp = a.y + ((int64_t)g * a.M + m) * a.O;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int c = o0 + ob + 16 * i + 4 * fq;
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

template <int K, int TM>
static void ws_launch(const C2WsArgs& a, bool dgrad, dim3 grid, size_t lds, hipStream_t s) {
  if (dgrad)
    hipLaunchKernelGGL((k_conv2d_ws<K, true, TM>), grid, dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((k_conv2d_ws<K, false, TM>), grid, dim3(256), lds, s, a);
}

// The slab rows of a tile of tm positions: the most samples it touches times the padded sample
static int64_t ws_rows(int tm, int B, int Ho, int Wo, int k) {
  const int64_t P = (int64_t)Ho * Wo;
  const int64_t ns = tm % P == 0 ? tm / P : P % tm == 0 ? 1 : (tm + 2 * P - 2) / P;
  return std::min<int64_t>(ns, B) * (Ho + k - 1) * (Wo + k - 1);
}

static bool ws_fits(int tm, int B, int Ho, int Wo, int k) {
  const int64_t rows = ws_rows(tm, B, Ho, Wo, k);
  return rows <= kWsMaxRows && 2 * (k * k * kWsTap + rows * kWsLd) <= 65536;
}

// G, B, H, W, cin, cout, k, pad describe the forward layer in both directions.  dgrad = 0: x is X [G*B][H][W][cs],
// y is Y [G*B][Ho][Wo][cout].  dgrad = 1: x is dY [G*B][Ho][Wo][cs], y is dX [G*B][H][W][cin], bias must be 0.  cs is
// the channel stride of the tensor read; w is client 0's fp32 [cout][cin][k][k] and ldw the client stride, bias
// client 0's fp32 [cout] (or 0) and ldb its client stride, both in elements.
void conv2d_ws(uintptr_t x, uintptr_t w, int64_t ldw, uintptr_t bias, int64_t ldb, uintptr_t y, int G, int B, int H,
               int W, int cin, int cs, int cout, int k, int pad, int dgrad, uintptr_t stream) {
  NIDT_REQUIRE(k >= 1 && k <= 3, "conv2d_ws: kernel size must be 1 .. 3");
  const int Ho = H + 2 * pad - k + 1, Wo = W + 2 * pad - k + 1;
  NIDT_REQUIRE(G > 0 && B > 0 && cin > 0 && cout > 0 && pad >= 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0,
               "conv2d_ws: G, B, cin, cout and both maps must be positive");
  NIDT_REQUIRE(!dgrad || (pad <= k - 1 && bias == 0), "conv2d_ws: the data gradient takes pad <= k - 1 and no bias");
  C2WsArgs a;
  a.x = ptr<const uint16_t>(x); a.w = ptr<const float>(w); a.bias = ptr<const float>(bias); a.y = ptr<uint16_t>(y);
  a.ldw = ldw; a.ldb = ldb;
  a.B = B; a.cs = cs; a.cin = cin;
  a.Hi = dgrad ? Ho : H; a.Wi = dgrad ? Wo : W; a.Ho = dgrad ? H : Ho; a.Wo = dgrad ? W : Wo;
  a.C = dgrad ? cout : cin; a.O = dgrad ? cin : cout; a.pad = dgrad ? k - 1 - pad : pad;
  NIDT_REQUIRE(a.C % 8 == 0 && cs % 8 == 0 && cs >= a.C,
               "conv2d_ws: the contraction channel count and its stride must be multiples of 8");
  NIDT_REQUIRE(x % 16 == 0 && w % 4 == 0 && bias % 4 == 0, "conv2d_ws: x must be 16-byte, w and bias 4-byte aligned");
  NIDT_REQUIRE((int64_t)cout * cin * k * k < (int64_t(1) << 31) && ldw >= (int64_t)cout * cin * k * k,
               "conv2d_ws: weight client stride below cout * cin * k * k");
  NIDT_REQUIRE(bias == 0 || ldb >= cout, "conv2d_ws: bias client stride below cout");
  NIDT_REQUIRE((int64_t)B * a.Ho * a.Wo < (int64_t(1) << 31) - 256 && (int64_t)B * a.Hi * a.Wi < (int64_t(1) << 31),
               "conv2d_ws: positions per client must fit 31 bits");
  a.M = B * a.Ho * a.Wo;
  a.nch = (a.C + kWsCK - 1) / kWsCK;
  a.Hp = a.Ho + k - 1; a.Wp = a.Wo + k - 1;
  NIDT_REQUIRE(ws_fits(64, B, a.Ho, a.Wo, k),
               "conv2d_ws: the padded samples of a tile exceed 768 slab rows or 64 KiB of LDS (small maps only)");
  const int tm = a.M >= 256 && ws_fits(256, B, a.Ho, a.Wo, k) ? 256 : 64;
  a.nrows = (int)ws_rows(tm, B, a.Ho, a.Wo, k);
  const size_t lds = sizeof(uint16_t) * ((size_t)k * k * kWsTap + (size_t)a.nrows * kWsLd);
  const int nm = (a.M + tm - 1) / tm, no = (a.O + 63) / 64;
  NIDT_REQUIRE(G <= 65535 && no <= 65535, "conv2d_ws: grid too large");
  const dim3 grid(nm, no, G);
  hipStream_t s = as_stream(stream);
  if (tm == 64) {
    switch (k) {
      case 1: ws_launch<1, 64>(a, dgrad, grid, lds, s); break;
      case 2: ws_launch<2, 64>(a, dgrad, grid, lds, s); break;
      default: ws_launch<3, 64>(a, dgrad, grid, lds, s); break;
    }
  } else {
    switch (k) {
      case 1: ws_launch<1, 256>(a, dgrad, grid, lds, s); break;
      case 2: ws_launch<2, 256>(a, dgrad, grid, lds, s); break;
      default: ws_launch<3, 256>(a, dgrad, grid, lds, s); break;
    }
  }
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
