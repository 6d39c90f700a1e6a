// Byzantine-robust aggregation over the client rows (BASELINE config 4): coordinate median / trimmed mean, and the
// pairwise squared distances and selection of (Multi-)Krum.
//
//   rows_order_mean  : out[j] = mean of the order statistics lo .. hi-1 of column j over the K listed rows
//   rows_pair_sqdist : D[i][k] (+)= sum_j ((double)(a_i[j] - a_k[j]))^2   (fp32 difference, exact fp64 square, fp64 sums)
//   krum_select      : score[i] = sum of the m smallest D[i][k], k != i; sel = the `multi` smallest scores
//
// All three read an fp32 row matrix through a base pointer, a row stride (16-B aligned rows, stride % 4 == 0) and an
// int32 device list ridx[K] of row numbers: the list gives the client order, the rows need not be contiguous, rows
// that are not listed and columns >= n are never read.  No atomics; every result is a function of the listed rows'
// contents, K and n only.
//
// One total order serves all of them ("a before b"): a < b; or b is NaN and a is not; or neither (equal values,
// -0 == +0, both NaN) and a comes first in the list.  It is evaluated on an integer key (order_key below) plus the
// list position, so a rank counted against it is exact and the ranks of a column are a permutation of 0 .. K-1.
// numpy / torch twins: engine/robust.py.
#include "common.h"

namespace nidt {

constexpr int kRobThreads = 256;
constexpr int kRobMaxK = 256;
constexpr int kPairTile = 64;        // pair tile: 64 x 64 rows, a 4 x 4 block of pairs per thread
constexpr int kPairCols = 64;        // columns per LDS stage
constexpr int kPairMaxChunks = 256;  // column chunks (blocks per pair tile) at most

// Monotone integer image of the order on floats: every NaN maps to the largest key (one above +inf's 0xff800000, so
// key + 1 never wraps), -0 and +0 to the same key.
constexpr uint32_t kNanKey = 0xff800001u;
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t b = __float_as_uint(v);
  if (v != v) return kNanKey;
  if (v == 0.f) return 0x80000000u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ uint64_t order_key_d(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  if (v != v) return ~0ull;
  if (v == 0.0) return 1ull << 63;
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// ---- order statistics per column ----
// One block ranks a tile of TC columns x K rows.  The rows' pieces are read coalesced (TC consecutive floats per row)
// into LDS, as values and as keys; the thread of (column c, row group g) then counts, for four of its rows at a time,
// how many of the column's K keys come before each (one conflict-free LDS read serves four comparisons), and leaves
// the ranks in a byte tile.  After a barrier the values are scattered to their rank slots (over the key tile, which
// is dead by then), and one thread per column adds the slots lo .. hi-1 in ascending rank: a sequential fp32 sum
// (additions only: nothing to contract) and one correctly rounded division.
// LDS: 9 bytes per element; K <= 128 takes TC = 64 and K <= 256 takes TC = 32: at most 72 KB, two blocks per CU.
template <int TC>
__global__ __launch_bounds__(kRobThreads) void k_rows_order_mean(const float* __restrict__ rows, int64_t stride,
                                                                 const int* __restrict__ ridx, int K, int64_t n, int lo,
                                                                 int hi, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rob_smem[];
  __shared__ int s_ridx[kRobMaxK];
  uint32_t* s_key = reinterpret_cast<uint32_t*>(rob_smem);          // [K][TC]
  float* s_sorted = reinterpret_cast<float*>(rob_smem);             // [K][TC], over the keys once they are dead
  float* s_val = reinterpret_cast<float*>(rob_smem) + (size_t)K * TC;  // [K][TC]
  uint8_t* s_rank = rob_smem + (size_t)K * TC * 8;                  // [K][TC]
  constexpr int G = kRobThreads / TC;  // row groups
  const int c = threadIdx.x & (TC - 1), g = threadIdx.x / TC;
  const int64_t col = (int64_t)blockIdx.x * TC + c;
  const bool live = col < n;
  for (int k = threadIdx.x; k < K; k += kRobThreads) s_ridx[k] = ridx[k];
  __syncthreads();
  for (int k = g; k < K; k += G) {
    const float v = live ? rows[(int64_t)s_ridx[k] * stride + col] : 0.f;
    s_val[k * TC + c] = v;
    s_key[k * TC + c] = order_key(v);
  }
  __syncthreads();
  if (live) {
    for (int k0 = g; k0 < K; k0 += 4 * G) {
      // row k comes before own row kk[u] iff key_k < key_u + (k < kk[u]): the rows kk[0] < kk[1] < ... cut the k loop
      // into five runs of constant thresholds, so a comparison is one compare and one add
      uint32_t me[4], th[4];
      int kk[4], r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        kk[u] = k0 + u * G;
        me[u] = kk[u] < K ? s_key[kk[u] * TC + c] : 0u;
        th[u] = me[u] + 1u;
        r[u] = 0;
      }
      int k = 0;
#pragma unroll
      for (int seg = 0; seg < 5; ++seg) {
        const int kend = (seg < 4 && kk[seg < 4 ? seg : 0] < K) ? kk[seg < 4 ? seg : 0] : K;
        for (; k < kend; ++k) {
          const uint32_t o = s_key[k * TC + c];
#pragma unroll
          for (int u = 0; u < 4; ++u) r[u] += (int)(o < th[u]);
        }
        if (seg < 4) th[seg] = me[seg];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kk[u] < K) s_rank[kk[u] * TC + c] = (uint8_t)r[u];
    }
  }
  __syncthreads();
  if (live)
    for (int k = g; k < K; k += G) s_sorted[(int)s_rank[k * TC + c] * TC + c] = s_val[k * TC + c];
  __syncthreads();
  if (live && g == 0) {
    float acc = s_sorted[lo * TC + c];
    for (int r = lo + 1; r < hi; ++r) acc = acc + s_sorted[r * TC + c];
    out[col] = __fdiv_rn(acc, (float)(hi - lo));
  }
}

void rows_order_mean(uintptr_t rows, int64_t stride, uintptr_t ridx, int64_t K, int64_t n, int64_t lo, int64_t hi,
                     uintptr_t out, uintptr_t stream) {
  NIDT_REQUIRE(stride % 4 == 0 && stride >= n && (rows & 15) == 0 && (ridx & 3) == 0 && (out & 3) == 0,
               "rows_order_mean: 16-byte aligned rows (stride % 4 == 0, stride >= n)");
  NIDT_REQUIRE(K >= 1 && K <= kRobMaxK && lo >= 0 && lo < hi && hi <= K && n >= 0 && rows != 0 && ridx != 0 && out != 0,
               "rows_order_mean: arguments (1 <= K <= 256, 0 <= lo < hi <= K)");
  if (n == 0) return;
  const int tc = K <= 128 ? 64 : 32;
  const int lds = (int)K * tc * 9;
  NIDT_REQUIRE((n + tc - 1) / tc < (int64_t(1) << 31), "rows_order_mean: n");
  const dim3 grid((unsigned)((n + tc - 1) / tc));
  hipStream_t st = as_stream(stream);
  if (tc == 64) {
    NIDT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rows_order_mean<64>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(k_rows_order_mean<64>, grid, dim3(kRobThreads), lds, st, ptr<const float>(rows), stride,
                       ptr<const int>(ridx), (int)K, n, (int)lo, (int)hi, ptr<float>(out));
  } else {
    NIDT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rows_order_mean<32>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(k_rows_order_mean<32>, grid, dim3(kRobThreads), lds, st, ptr<const float>(rows), stride,
                       ptr<const int>(ridx), (int)K, n, (int)lo, (int)hi, ptr<float>(out));
  }
  NIDT_CHECK(hipGetLastError());
}

// ---- pairwise squared distances ----
// columns per block: a function of n only (never of K or of the row list), so a pair's partial sums - and its
// distance - are the same bits whichever rows share the launch.  8192 columns per block, at most kPairMaxChunks
// blocks per pair tile (then a multiple of the 64-column stage).
static int64_t pair_chunk(int64_t n, int* nchunk) {
  int64_t chunk = 8192;
  int64_t nc = (n + chunk - 1) / chunk;
  if (nc > kPairMaxChunks) {
    chunk = ((n + kPairMaxChunks - 1) / kPairMaxChunks + kPairCols - 1) & ~int64_t(kPairCols - 1);
    nc = (n + chunk - 1) / chunk;
  }
  *nchunk = (int)(nc > 0 ? nc : 1);
  return chunk;
}

static int pair_tiles(int64_t K) {
  const int nT = (int)((K + kPairTile - 1) / kPairTile);
  return nT * (nT + 1) / 2;  // the upper triangle of the tile grid: D is symmetric
}

// doubles of workspace for rows_pair_sqdist(K, n): one 64 x 64 partial per (column chunk, pair tile)
int64_t rows_pair_sqdist_workspace(int64_t K, int64_t n) {
  int nc;
  pair_chunk(n, &nc);
  return (int64_t)nc * pair_tiles(K) * kPairTile * kPairTile;
}

// tile t of the upper triangle -> (I, J), I <= J
__device__ __forceinline__ void pair_tile_of(int t, int nT, int* I, int* J) {
  int i = 0;
  while (t >= nT - i) {
    t -= nT - i;
    ++i;
  }
  *I = i;
  *J = i + t;
}

// grid (column chunks, pair tiles).  Block (b, t) owns the pairs (I-tile row, J-tile row) over the columns
// [b * chunk, (b + 1) * chunk) ∩ [0, n): 64 columns of the 64 + 64 rows are staged per step into LDS as [column][row]
// (the next step's 16-B global loads are in flight while this one is summed), and thread (ti, tj) reads four
// consecutive rows of either tile with one 16-B LDS read per column for its 4 x 4 pairs: 16 fp32 subtractions,
// conversions and fp64 FMAs (the square of an fp32 value is exact in fp64, so the FMA rounds once, as acc + d * d does)
// against two LDS reads, each pair's sum in column order.  Rows past K and columns past the chunk are staged as 0
// (difference 0).  One fp64 partial per (chunk, tile, pair).
__global__ __launch_bounds__(kRobThreads) void k_rows_pair_sqdist(const float* __restrict__ rows, int64_t stride,
                                                                  const int* __restrict__ ridx, int K, int64_t n,
                                                                  int64_t chunk, double* __restrict__ part, int ntiles) {
  __shared__ __attribute__((aligned(16))) float sA[kPairCols * kPairTile];
  __shared__ __attribute__((aligned(16))) float sB[kPairCols * kPairTile];
  int I, J;
  pair_tile_of(blockIdx.y, (K + kPairTile - 1) / kPairTile, &I, &J);
  const int64_t s = (int64_t)blockIdx.x * chunk;
  const int64_t e = s + chunk < n ? s + chunk : n;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, r16 = l & 15, cq = l >> 4;
  // staging: wave w loads rows 32 w .. 32 w + 31 of the 128 (I tile, then J tile), lane (r16, cq) the 16-B piece cq
  // of row r16 in each of four 16-column blocks
  float* S = w < 2 ? sA : sB;
  const float* rp[2];
  int lr[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    lr[h] = ((w & 1) * 2 + h) * 16 + r16;
    const int gr = (w < 2 ? I : J) * kPairTile + lr[h];
    rp[h] = gr < K ? rows + (int64_t)ridx[gr] * stride : nullptr;
  }
  float4 g[8];
  auto load = [&](int64_t c0) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int64_t col = c0 + (it & 3) * 16 + cq * 4;
      const float* p = rp[it >> 2];
      g[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p != nullptr) {
        if (col + 3 < e) {
          g[it] = *reinterpret_cast<const float4*>(p + col);
        } else {
          if (col < e) g[it].x = p[col];
          if (col + 1 < e) g[it].y = p[col + 1];
          if (col + 2 < e) g[it].z = p[col + 2];
        }
      }
    }
  };
  const int ti = threadIdx.x & 15, tj = threadIdx.x >> 4;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  if (s < e) load(s);
  for (int64_t c0 = s; c0 < e; c0 += kPairCols) {
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      float* d = S + ((it & 3) * 16 + cq * 4) * kPairTile + lr[it >> 2];
      d[0] = g[it].x;
      d[kPairTile] = g[it].y;
      d[2 * kPairTile] = g[it].z;
      d[3 * kPairTile] = g[it].w;
    }
    __syncthreads();
    if (c0 + kPairCols < e) load(c0 + kPairCols);
    const int nc = e - c0 < kPairCols ? (int)(e - c0) : kPairCols;
    for (int c = 0; c < nc; ++c) {
      const float4 va = *reinterpret_cast<const float4*>(sA + c * kPairTile + 4 * ti);
      const float4 vb = *reinterpret_cast<const float4*>(sB + c * kPairTile + 4 * tj);
      const float a4[4] = {va.x, va.y, va.z, va.w}, b4[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double d = (double)(a4[a] - b4[b]);
          acc[a][b] = fma(d, d, acc[a][b]);
        }
    }
  }
  double* pt = part + ((int64_t)blockIdx.x * ntiles + blockIdx.y) * (kPairTile * kPairTile);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) pt[(4 * ti + a) * kPairTile + 4 * tj + b] = acc[a][b];
}

// One thread per (tile, pair): the pair's partials are added in chunk order (coalesced over the pairs), then written -
// or added, with accumulate - to D[i][k] and, from an off-diagonal tile, to D[k][i] (a diagonal tile computes both
// itself: fl(a - b) = -fl(b - a), so the two are the same bits).  The diagonal is exactly 0 (an Inf row would make
// Inf - Inf = NaN of it).
__global__ __launch_bounds__(kRobThreads) void k_rows_pair_finish(const double* __restrict__ part, int nchunk, int ntiles,
                                                                  int K, double* __restrict__ D, int accumulate) {
  const int idx = blockIdx.x * kRobThreads + threadIdx.x;
  const int t = idx / (kPairTile * kPairTile), el = idx % (kPairTile * kPairTile);
  if (t >= ntiles) return;
  int I, J;
  pair_tile_of(t, (K + kPairTile - 1) / kPairTile, &I, &J);
  const int i = I * kPairTile + el / kPairTile, k = J * kPairTile + el % kPairTile;
  if (i >= K || k >= K) return;
  if (i == k) {
    if (!accumulate) D[(int64_t)i * K + i] = 0.0;
    return;
  }
  double sum = 0.0;
  for (int b = 0; b < nchunk; ++b) sum += part[((int64_t)b * ntiles + t) * (kPairTile * kPairTile) + el];
  double* d0 = D + (int64_t)i * K + k;
  *d0 = accumulate ? *d0 + sum : sum;
  if (I != J) {
    double* d1 = D + (int64_t)k * K + i;
    *d1 = accumulate ? *d1 + sum : sum;
  }
}

void rows_pair_sqdist(uintptr_t rows, int64_t stride, uintptr_t ridx, int64_t K, int64_t n, uintptr_t part,
                      uintptr_t D, int64_t accumulate, uintptr_t stream) {
  NIDT_REQUIRE(stride % 4 == 0 && stride >= n && (rows & 15) == 0 && (ridx & 3) == 0 && (part & 7) == 0 &&
                   (D & 7) == 0,
               "rows_pair_sqdist: 16-byte aligned rows (stride % 4 == 0, stride >= n)");
  NIDT_REQUIRE(K >= 1 && K <= kRobMaxK && n >= 0 && rows != 0 && ridx != 0 && part != 0 && D != 0,
               "rows_pair_sqdist: arguments (1 <= K <= 256)");
  int nchunk;
  const int64_t chunk = pair_chunk(n, &nchunk);
  const int ntiles = pair_tiles(K);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_rows_pair_sqdist, dim3(nchunk, ntiles), dim3(kRobThreads), 0, st, ptr<const float>(rows), stride,
                     ptr<const int>(ridx), (int)K, n, chunk, ptr<double>(part), ntiles);
  hipLaunchKernelGGL(k_rows_pair_finish, dim3(ntiles * kPairTile * kPairTile / kRobThreads), dim3(kRobThreads), 0, st,
                     ptr<const double>(part), nchunk, ntiles, (int)K, ptr<double>(D), (int)(accumulate != 0));
  NIDT_CHECK(hipGetLastError());
}

// ---- Krum scores and selection ----
// Block i ranks row i of D (without the diagonal) by counting under the order above, scatters the values to their
// rank slots, and one thread adds the first min(m, K - 1) of them in ascending order in fp64.
__global__ __launch_bounds__(kRobThreads) void k_krum_scores(const double* __restrict__ D, int K, int m,
                                                             double* __restrict__ score) {
  __shared__ uint64_t s_key[kRobMaxK];
  __shared__ double s_sorted[kRobMaxK];
  const int i = blockIdx.x, k = threadIdx.x;
  double v = 0.0;
  uint64_t key = ~0ull;
  if (k < K) {
    v = D[(int64_t)i * K + k];
    key = order_key_d(v);
    s_key[k] = key;
  }
  __syncthreads();
  if (k < K && k != i) {
    int r = 0;
    for (int q = 0; q < K; ++q) {
      const uint64_t o = s_key[q];
      r += (int)((q != i) & ((o < key) | ((o == key) & (q < k))));
    }
    s_sorted[r] = v;
  }
  __syncthreads();
  if (k == 0) {
    const int mm = m < K - 1 ? m : K - 1;
    double t = 0.0;
    for (int r = 0; r < mm; ++r) t += s_sorted[r];
    score[i] = t;
  }
}

// one block: the `multi` smallest scores, in ascending order, under the same order
__global__ __launch_bounds__(kRobThreads) void k_krum_pick(const double* __restrict__ score, int K, int multi,
                                                           int* __restrict__ sel) {
  __shared__ uint64_t s_key[kRobMaxK];
  const int k = threadIdx.x;
  uint64_t key = ~0ull;
  if (k < K) {
    key = order_key_d(score[k]);
    s_key[k] = key;
  }
  __syncthreads();
  if (k < K) {
    int r = 0;
    for (int q = 0; q < K; ++q) {
      const uint64_t o = s_key[q];
      r += (int)((o < key) | ((o == key) & (q < k)));
    }
    if (r < multi) sel[r] = k;
  }
}

void krum_select(uintptr_t D, int64_t K, int64_t f, int64_t multi, uintptr_t sel, uintptr_t score, uintptr_t stream) {
  NIDT_REQUIRE(K >= 1 && K <= kRobMaxK && f >= 0 && multi >= 1 && multi <= K && D != 0 && sel != 0 && score != 0 &&
                   (D & 7) == 0 && (score & 7) == 0 && (sel & 3) == 0,
               "krum_select: arguments (1 <= K <= 256, f >= 0, 1 <= multi <= K)");
  const int64_t m = K - f - 2 > 1 ? K - f - 2 : 1;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_krum_scores, dim3((unsigned)K), dim3(kRobThreads), 0, st, ptr<const double>(D), (int)K, (int)m,
                     ptr<double>(score));
  hipLaunchKernelGGL(k_krum_pick, dim3(1), dim3(kRobThreads), 0, st, ptr<const double>(score), (int)K, (int)multi,
                     ptr<int>(sel));
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
