// Client-grouped Linear layers of the small 2-D image models (lenet5, cnn_cifar10/100, vgg11 classifiers — reference
// fedml_api/model/cv/{lenet5,cnn_cifar10,vgg}.py), replacing the batched library GEMM of the batched 2-D engine:
//     Y [g][b][n] = bf16(sum_k X [g][b][k] bf16(W[g][n][k]) + bias[g][n])          forward
//     dX[g][b][k] = bf16(sum_n dY[g][b][n] bf16(W[g][n][k]))                       data gradient
//     dW[g][n][k] =      sum_b dY[g][b][n] X[g][b][k],  dB[g][n] = sum_b dY[g][b][n]   weight / bias gradient (fp32)
// X / dY / Y / dX are contiguous bf16 rows [G*B][K or N]; W / bias / dW / dB are fp32 blocks at a client stride, read
// and written where they lie in the parameter / gradient rows (4-byte alignment only).  B = 4..128 rows reuse each
// weight, so all three are bound by the fp32 weight (or weight-gradient) traffic: every weight is read from global
// memory exactly once per (batch tile, kernel), as fp32, and is never written back in any form.
//
//  * all three: 16x16x32 bf16 MFMA, fp32 accumulators, block = 4 waves = 64 x 64 output tile, wave = 32 x 32;
//  * forward and data gradient are ONE kernel (k_linear_g<DGRAD, VEC>): both walk 64 x 64 fp32 tiles of W[n][k] (forward
//    along k at fixed n-tile, data gradient along n at fixed k-tile).  A tile is fetched as lane-consecutive dwords
//    along k (16 per thread, coalesced whatever the block's offset), rounded to bf16 in registers (hardware RNE) and
//    stored [n][k] into one of two LDS buffers; the next tile's global loads (and the next activation fragments') are
//    issued before the current tile's MFMAs, one barrier per tile.  64 k per tile instead of the suggested 32: a lane
//    row is then a 256-B run, and 16 independent loads per thread are in flight;
//  * the forward reads its weight fragment (8 consecutive k of one n) as one 16-B LDS read; the data gradient needs
//    8 consecutive n of one k from the same [n][k] tile and reads it with ds_read_b64_tr_b16 (the transposing read of
//    the conv weight gradients) — the tile is NOT stored transposed, so both directions share the staging code;
//  * the activation fragment (8 consecutive contraction elements of one row) comes straight from global memory: one
//    16-B load when the row length is a multiple of 8 (VEC), element loads otherwise;
//  * outputs: a lane holds 4 consecutive output columns of one row -> one 8-B bf16 store when the row length allows;
//  * weight gradient: grid (k-tile, n-tile, client); the contraction runs over b (zero padded to 32), both operands are
//    row-major in the other index, so 32-row tiles of dY and X go through LDS (16-B stores, register prefetch, two
//    buffers) and both fragments are transposing reads.  dY is the A operand: a lane's 4 accumulator rows are n and
//    the 16 lanes of a row hold consecutive k (64-B fp32 store runs).  The k-tile-0 blocks also sum their dY tile
//    columns in fp32, b ascending, into dB.  One block owns each output element: no atomics, no split over b.
// Rows of the LDS tiles are padded to 72 bf16 (144 B = 36 banks): 16-B aligned for the vector accesses, and the rows
// of a fragment read do not all start on the same bank as 128-B rows would.
// Measured (profiles/r10_linear_g.txt): 3.3-5.5 TB/s of fp32 weight bytes on the two large layers at 100 clients, in
// back-to-back calls on the same 150-245 MB of weights, which the 256 MB Infinity Cache can hold: re-read rates, not
// shown to be HBM streaming rates.  The few-client, long-contraction case (1600 -> 384 at G = 8: 48 blocks x 25 serial
// tiles) is latency-bound and would want a split over the contraction, which nothing in the zoo's step time asks for
// yet.
#include "common.h"

namespace nidt {

constexpr int kLgLd = 72;  // LDS row stride in bf16 elements

// 8 consecutive elements c .. c + 7 of a bf16 row of length L (zeros past L, or when !valid)
template <bool VEC>
__device__ __forceinline__ bf16x8 lg_ld8(const uint16_t* row, bool valid, int L, int c) {
  bf16x8 v = {};
  if (!valid || c >= L) return v;
  if (VEC) return *reinterpret_cast<const bf16x8*>(row + c);
  uint16_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = c + j < L ? row[c + j] : (uint16_t)0;
  return __builtin_bit_cast(bf16x8, make_uint4(e[0] | (uint32_t)e[1] << 16, e[2] | (uint32_t)e[3] << 16,
                                               e[4] | (uint32_t)e[5] << 16, e[6] | (uint32_t)e[7] << 16));
}

// MFMA fragment with the contraction along the ROWS of an LDS tile [row][kLgLd]: lane (fr, fq) gets column c0 + fr,
// rows r0 + 8 fq .. + 7.  Within a 16-lane group, lane 4 qq + pp hands ds_read_b64_tr_b16 the address of row qq,
// columns 4 pp .. + 3 and receives column (lane & 15) of those 4 rows (k_wgrad1x1's frag).
__device__ __forceinline__ bf16x8 lg_tr_frag(const uint16_t* tile, int r0, int c0, int lane) {
  typedef short v4s __attribute__((ext_vector_type(4)));
  typedef short v8s __attribute__((ext_vector_type(8)));
  const int li = lane & 15;
  const uint16_t* p = tile + (r0 + 8 * (lane >> 4) + (li >> 2)) * kLgLd + c0 + 4 * (li & 3);
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p + 4 * kLgLd));
  const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

struct LgArgs {
  const uint16_t* a;  // forward: x [G*B][K]; data gradient: dy [G*B][N]
  const float* w;     // client 0's [N][K]
  const float* bias;  // client 0's [N] or null (forward only)
  uint16_t* out;      // forward: y [G*B][N]; data gradient: dx [G*B][K]
  int64_t ldw, ldb;   // client strides in elements
  int G, B, K, N;
};

// out[g][b][o] = sum_l a[g][b][l] * (DGRAD ? W[g][l][o] : W[g][o][l]) (+ bias[g][o]);  VEC: the rows of `a` are whole
// aligned 16-B pieces (contraction length % 8 == 0)
template <bool DGRAD, bool VEC>
__global__ __launch_bounds__(256) void k_linear_g(LgArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t sW[2][64 * kLgLd];
  const int g = blockIdx.z, o0 = blockIdx.y * 64;
  const int L = DGRAD ? a.N : a.K, O = DGRAD ? a.K : a.N;  // contraction length, output row length
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wp = wid & 1, wc = wid >> 1;  // wave: batch rows half wp, output columns half wc
  const int bb = blockIdx.x * 64 + wp * 32;
  const float* wg = a.w + (int64_t)g * a.ldw;
  // this lane's two B-operand columns (batch rows bb + fr, bb + 16 + fr)
  const uint16_t* arow[2];
  bool bval[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int b = bb + 16 * j + fr;
    bval[j] = b < a.B;
    arow[j] = a.a + ((int64_t)g * a.B + (bval[j] ? b : 0)) * L;
  }
  const int sc = tid & 63, sr = tid >> 6;  // staging: k column sc, n rows sr + 4 i of the 64 x 64 weight tile
  float wr[16];
  bf16x8 xn[2][2];
  auto fetch = [&](int s) {  // contraction step s: weights into wr, activation fragments into xn
    const int l0 = 64 * s;
    const int k = DGRAD ? o0 + sc : l0 + sc;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int n = (DGRAD ? l0 : o0) + sr + 4 * i;
      wr[i] = n < a.N && k < a.K ? wg[(int64_t)n * a.K + k] : 0.f;
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j) xn[kk][j] = lg_ld8<VEC>(arow[j], bval[j], L, l0 + 32 * kk + 8 * fq);
  };
  f32x4 acc[2][2] = {};
  const int ns = (L + 63) / 64;
  fetch(0);
  for (int s = 0; s < ns; ++s) {
    uint16_t* sb = sW[s & 1];  // its readers of step s - 2 are all past the barrier of step s - 1
#pragma unroll
    for (int i = 0; i < 16; ++i) sb[(sr + 4 * i) * kLgLd + sc] = f32_to_bf16(wr[i]);
    bf16x8 xc[2][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j) xc[kk][j] = xn[kk][j];
    __syncthreads();
    if (s + 1 < ns) fetch(s + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 fa[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int oc = wc * 32 + 16 * i;
        fa[i] = DGRAD ? lg_tr_frag(sb, 32 * kk, oc, lane)
                      : *reinterpret_cast<const bf16x8*>(sb + (oc + fr) * kLgLd + 32 * kk + 8 * fq);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], xc[kk][j], acc[i][j], 0, 0, 0);
    }
  }
  // lane: output columns o0 + wc 32 + 16 i + 4 fq + r (r = 0..3) of batch row bb + 16 j + fr
  const float* bias = a.bias ? a.bias + (int64_t)g * a.ldb : nullptr;
  const bool pk = (O & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 7) == 0;  // rows of whole aligned 8-B pieces
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int b = bb + 16 * j + fr;
    if (b >= a.B) continue;
    uint16_t* op = a.out + ((int64_t)g * a.B + b) * O;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = o0 + wc * 32 + 16 * i + 4 * fq;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + (bias && c + r < O ? bias[c + r] : 0.f);
      if (pk && c + 3 < O) {
        *reinterpret_cast<uint2*>(op + c) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (c + r < O) op[c + r] = f32_to_bf16(v[r]);
      }
    }
  }
}

struct LgWgArgs {
  const uint16_t* x;   // [G*B][K]
  const uint16_t* dy;  // [G*B][N]
  float* dw;           // client 0's [N][K]
  float* db;           // client 0's [N] or null
  int64_t lddw, lddb;  // client strides in elements
  int G, B, K, N;
};

// VX / VD: the x / dy rows are whole aligned 16-B pieces (K % 8 == 0 / N % 8 == 0)
template <bool VX, bool VD>
__global__ __launch_bounds__(256) void k_linear_g_wgrad(LgWgArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t sD[2][32 * kLgLd];
  __shared__ __attribute__((aligned(16))) uint16_t sX[2][32 * kLgLd];
  const int g = blockIdx.z, n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int wn = wid & 1, wk = wid >> 1;       // wave: n half wn, k half wk
  const int sr = tid >> 3, sc = (tid & 7) * 8;  // staging: batch row sr, columns sc .. sc + 7 of both 32 x 64 tiles
  const uint16_t* xg = a.x + (int64_t)g * a.B * a.K;
  const uint16_t* dg = a.dy + (int64_t)g * a.B * a.N;
  const bool bias_blk = a.db && blockIdx.x == 0;  // block-uniform
  bf16x8 rd, rx;
  auto fetch = [&](int s) {
    const int b = 32 * s + sr;
    rd = lg_ld8<VD>(dg + (int64_t)(b < a.B ? b : 0) * a.N, b < a.B, a.N, n0 + sc);
    rx = lg_ld8<VX>(xg + (int64_t)(b < a.B ? b : 0) * a.K, b < a.B, a.K, k0 + sc);
  };
  f32x4 acc[2][2] = {};
  float dbs = 0.f;
  const int ns = (a.B + 31) / 32;
  fetch(0);
  for (int s = 0; s < ns; ++s) {
    uint16_t* bd = sD[s & 1];
    uint16_t* bx = sX[s & 1];
    *reinterpret_cast<bf16x8*>(bd + sr * kLgLd + sc) = rd;
    *reinterpret_cast<bf16x8*>(bx + sr * kLgLd + sc) = rx;
    __syncthreads();
    if (s + 1 < ns) fetch(s + 1);
    bf16x8 fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = lg_tr_frag(bd, 0, wn * 32 + 16 * i, lane);
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = lg_tr_frag(bx, 0, wk * 32 + 16 * j, lane);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    if (bias_blk && tid < 64) {  // column n0 + tid of the staged dY rows, b ascending (padding rows are zeros)
#pragma unroll 8
      for (int r = 0; r < 32; ++r) dbs += bf16_to_f32(bd[r * kLgLd + tid]);
    }
  }
  // lane: rows n0 + wn 32 + 16 i + 4 fq + r, column k0 + wk 32 + 16 j + fr
  float* dwg = a.dw + (int64_t)g * a.lddw;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wn * 32 + 16 * i + 4 * fq + r;
      if (n >= a.N) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int k = k0 + wk * 32 + 16 * j + fr;
        if (k < a.K) dwg[(int64_t)n * a.K + k] = acc[i][j][r];
      }
    }
  if (bias_blk && tid < 64 && n0 + tid < a.N) a.db[(int64_t)g * a.lddb + n0 + tid] = dbs;
}

static void lg_require(const char* who, int G, int B, int K, int N, int64_t ldw, bool has_b, int64_t ldb) {
  const std::string p(who);
  NIDT_REQUIRE(G > 0 && B > 0 && K > 0 && N > 0, p + ": G, B, K, N must be positive");
  NIDT_REQUIRE(G <= 65535 && (N + 63) / 64 <= 65535 && (K + 63) / 64 <= 65535, p + ": grid too large");
  NIDT_REQUIRE(ldw >= (int64_t)N * K, p + ": weight client stride below N * K");
  NIDT_REQUIRE(!has_b || ldb >= N, p + ": bias client stride below N");
}

static bool lg_vec(uintptr_t p, int L) { return L % 8 == 0 && p % 16 == 0; }

template <bool DGRAD>
static void lg_launch(const LgArgs& a, uintptr_t act, hipStream_t s) {
  const int L = DGRAD ? a.N : a.K, O = DGRAD ? a.K : a.N;
  const dim3 grid((a.B + 63) / 64, (O + 63) / 64, a.G);
  if (lg_vec(act, L))
    hipLaunchKernelGGL((k_linear_g<DGRAD, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((k_linear_g<DGRAD, false>), grid, dim3(256), 0, s, a);
  NIDT_CHECK(hipGetLastError());
}

void linear_g_fwd(uintptr_t x, uintptr_t w, int64_t ldw, uintptr_t bias, int64_t ldb, uintptr_t y, int G, int B, int K,
                  int N, uintptr_t stream) {
  lg_require("linear_g_fwd", G, B, K, N, ldw, bias != 0, ldb);
  LgArgs a;
  a.a = ptr<const uint16_t>(x); a.w = ptr<const float>(w); a.bias = ptr<const float>(bias); a.out = ptr<uint16_t>(y);
  a.ldw = ldw; a.ldb = ldb; a.G = G; a.B = B; a.K = K; a.N = N;
  lg_launch<false>(a, x, as_stream(stream));
}

void linear_g_dgrad(uintptr_t dy, uintptr_t w, int64_t ldw, uintptr_t dx, int G, int B, int K, int N,
                    uintptr_t stream) {
  lg_require("linear_g_dgrad", G, B, K, N, ldw, false, 0);
  LgArgs a;
  a.a = ptr<const uint16_t>(dy); a.w = ptr<const float>(w); a.bias = nullptr; a.out = ptr<uint16_t>(dx);
  a.ldw = ldw; a.ldb = 0; a.G = G; a.B = B; a.K = K; a.N = N;
  lg_launch<true>(a, dy, as_stream(stream));
}

// db may be 0 (no bias gradient)
void linear_g_wgrad(uintptr_t x, uintptr_t dy, uintptr_t dw, int64_t lddw, uintptr_t db, int64_t lddb, int G, int B,
                    int K, int N, uintptr_t stream) {
  lg_require("linear_g_wgrad", G, B, K, N, lddw, db != 0, lddb);
  LgWgArgs a;
  a.x = ptr<const uint16_t>(x); a.dy = ptr<const uint16_t>(dy); a.dw = ptr<float>(dw); a.db = ptr<float>(db);
  a.lddw = lddw; a.lddb = lddb; a.G = G; a.B = B; a.K = K; a.N = N;
  const dim3 grid((K + 63) / 64, (N + 63) / 64, G);
  hipStream_t s = as_stream(stream);
  const bool vx = lg_vec(x, K), vd = lg_vec(dy, N);
  if (vx && vd) hipLaunchKernelGGL((k_linear_g_wgrad<true, true>), grid, dim3(256), 0, s, a);
  else if (vx) hipLaunchKernelGGL((k_linear_g_wgrad<true, false>), grid, dim3(256), 0, s, a);
  else if (vd) hipLaunchKernelGGL((k_linear_g_wgrad<false, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_linear_g_wgrad<false, false>), grid, dim3(256), 0, s, a);
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
