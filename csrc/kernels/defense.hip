// Norm-difference clipping and weak-DP noise on the client rows (the reference's RobustAggregator,
// fedml_core/robustness/robust_aggregation.py:32-55), fused into the FedAvg weighted row sum.
//
//   rows_diff_norm   : norm[c] = || rows[c, :P] - ref[:P] ||_2            (one streaming pass, fp64 accumulation)
//   clipped_rows_sum : out[j]  = sum_c wts[c] * ( (rows[c][j] - ref[j]) / max(1, norm[c] / bound) + ref[j]
//                                                 + stddev * z(seed, cids[c], j) )         (one streaming pass)
//
// rows is the [C, ld] fp32 client matrix (16-B aligned rows, columns [P, ld) are padding and are never read), ref
// the global model [P].  Both kernels are deterministic and free of atomics; every per-row quantity is a function of
// (P, row contents) only, so results do not depend on how clients are sharded over ranks.
//
// The noise z(seed, cid, j) is a counter-based unit normal (Box-Muller over two splitmix hashes of
// (seed, client id, coordinate)): any rank, launch shape or row order draws the same value for the same client and
// coordinate.  numpy twin: engine/defense.py noise_z_np.
#include "common.h"

namespace nidt {

constexpr int kDefThreads = 256;
constexpr int kDefMaxBlocks = 1024;  // norm-pass blocks per row at most (the finish kernel stages them in LDS)
constexpr int kDefRows = 8;  // rows per block in the norm pass (they share one register copy of ref's piece)
constexpr int kDefVec = 8;   // 16-B pieces per thread per step of the norm pass: 256 x 4 x 8 = 8192 columns

// the splitmix finaliser of sparse.hip (numpy twin: engine/masks.py _mix_hash_np)
__device__ __forceinline__ uint32_t def_mix_hash(uint64_t seed, uint32_t a, uint32_t b) {
  uint64_t z = seed ^ (0x9e3779b97f4a7c15ull * (((uint64_t)a << 32) ^ (uint64_t)b));
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}

// u1 in (0, 1], u2 in [0, 1) on the 2^-24 grid (both exact in fp32); accurate logf / sqrtf / cospif (no fast math)
__device__ __forceinline__ float noise_z(uint64_t seed, uint32_t cid, uint32_t j) {
  const uint32_t h1 = def_mix_hash(seed, cid, j);
  const uint32_t h2 = def_mix_hash(seed ^ 0x5bd1e995ull, cid, j);
  const float u1 = (float)((h1 >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(h2 >> 8) * 0x1p-24f;
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// blocks per row: a function of P only (never of C), so a row's partial sums - and its norm - are the same bits
// whichever rows share the launch.  8192 columns per block (256 threads x 4 floats x kDefVec), at most kDefMaxBlocks
// blocks per row.
static int64_t def_chunk(int64_t P, int* nblk) {
  int64_t chunk = 8192;
  int64_t nb = (P + chunk - 1) / chunk;
  if (nb > kDefMaxBlocks) {
    chunk = ((P + kDefMaxBlocks - 1) / kDefMaxBlocks + 3) & ~int64_t(3);
    nb = (P + chunk - 1) / chunk;
  }
  *nblk = (int)(nb > 0 ? nb : 1);
  return chunk;
}

int64_t rows_diff_norm_blocks(int64_t P) {
  int nb;
  def_chunk(P, &nb);
  return nb;
}

// grid (nblk, ceil(C / kDefRows)): block (b, q) sums (rows[c][j] - ref[j])^2 over j in [b * chunk, (b + 1) * chunk) ∩
// [0, P) for the rows c of group q.  ref's piece is loaded once per block into registers and shared by the group's
// rows: with one row per block ref (10 MB for AlexNet3D, more than an XCD's L2) came back over the fabric for every
// row and the pass moved twice the rows' bytes (measured 2.5 TB/s of row bytes against 5.3 TB/s for
// k_weighted_rows_sum).  The difference is an fp32 subtraction (the reference subtracts fp32 tensors); its square is
// exact in fp64 and the sums are fp64, each thread's in index order, then reduced over the block in a fixed order.
// The partial of (row, block) does not depend on which rows share the launch.  One fp64 partial per (row, block), no
// atomics.
__global__ __launch_bounds__(kDefThreads) void k_rows_diff_sqnorm(const float* __restrict__ rows,
                                                                  const float* __restrict__ ref, int C, int64_t P,
                                                                  int64_t stride, int64_t chunk,
                                                                  double* __restrict__ part, int nblk) {
  __shared__ double red[kDefRows][kDefThreads / 64];
  const int c0 = blockIdx.y * kDefRows;
  const int nr = C - c0 < kDefRows ? C - c0 : kDefRows;
  const float* row0 = rows + (int64_t)c0 * stride;
  const int64_t s = (int64_t)blockIdx.x * chunk;
  const int64_t e = s + chunk < P ? s + chunk : P;
  const int64_t e4 = s + ((e - s) & ~int64_t(3));
  double acc[kDefRows];
#pragma unroll
  for (int r = 0; r < kDefRows; ++r) acc[r] = 0.0;
  for (int64_t base = s + 4 * threadIdx.x; base < e4; base += 4 * kDefThreads * kDefVec) {
    float4 g[kDefVec];
#pragma unroll
    for (int u = 0; u < kDefVec; ++u) {
      const int64_t i = base + (int64_t)u * 4 * kDefThreads;
      g[u] = i < e4 ? *reinterpret_cast<const float4*>(ref + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int r = 0; r < kDefRows; ++r) {
      if (r < nr) {  // block uniform
        const float* row = row0 + (int64_t)r * stride;
        float4 v[kDefVec];
#pragma unroll
        for (int u = 0; u < kDefVec; ++u) {  // kDefVec 16-B loads in flight before the first use
          const int64_t i = base + (int64_t)u * 4 * kDefThreads;
          v[u] = i < e4 ? *reinterpret_cast<const float4*>(row + i) : g[u];  // past the end: difference 0
        }
#pragma unroll
        for (int u = 0; u < kDefVec; ++u) {
          const double dx = (double)(v[u].x - g[u].x), dy = (double)(v[u].y - g[u].y),
                       dz = (double)(v[u].z - g[u].z), dw = (double)(v[u].w - g[u].w);
          acc[r] = fma(dx, dx, acc[r]);
          acc[r] = fma(dy, dy, acc[r]);
          acc[r] = fma(dz, dz, acc[r]);
          acc[r] = fma(dw, dw, acc[r]);
        }
      }
    }
  }
  for (int64_t i = e4 + threadIdx.x; i < e; i += kDefThreads) {  // the row's last P % 4 columns (last block only)
    const float gi = ref[i];
#pragma unroll
    for (int r = 0; r < kDefRows; ++r) {
      if (r < nr) {
        const double d = (double)(row0[(int64_t)r * stride + i] - gi);
        acc[r] = fma(d, d, acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kDefRows; ++r) {
    const double t = wave_sum_d(acc[r]);
    if ((threadIdx.x & 63) == 0) red[r][threadIdx.x >> 6] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < nr) {
    double t = red[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < kDefThreads / 64; ++w) t += red[threadIdx.x][w];
    part[(int64_t)(c0 + threadIdx.x) * nblk + blockIdx.x] = t;
  }
}

// one block per row: the row's partials (nblk <= kDefMaxBlocks) are staged in LDS with coalesced loads, then summed by
// one thread in index order in fp64; sqrt in fp64, one cast to fp32.  (One thread reading its row's partials straight
// from global memory was a chain of ~300 load latencies: 0.1 ms for AlexNet3D rows, as long as the streaming pass.)
__global__ __launch_bounds__(kDefThreads) void k_rows_norm_finish(const double* __restrict__ part, int nblk,
                                                                  float* __restrict__ norm) {
  __shared__ double sp[kDefMaxBlocks];
  const int c = blockIdx.x;
  const double* p = part + (int64_t)c * nblk;
  for (int b = threadIdx.x; b < nblk; b += kDefThreads) sp[b] = p[b];
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int b = 0; b < nblk; ++b) t += sp[b];
    norm[c] = (float)sqrt(t);
  }
}

void rows_diff_norm(uintptr_t rows, uintptr_t ref, int64_t C, int64_t P, int64_t stride, uintptr_t part,
                    uintptr_t norm, uintptr_t stream) {
  NIDT_REQUIRE(stride % 4 == 0 && stride >= P && (rows & 15) == 0 && (ref & 15) == 0 && (part & 7) == 0,
               "rows_diff_norm: 16-byte aligned rows and ref (stride % 4 == 0, stride >= P)");
  NIDT_REQUIRE(C >= 0 && C <= 65535 * kDefRows && P >= 0 && rows != 0 && ref != 0 && part != 0 && norm != 0,
               "rows_diff_norm: arguments");
  if (C == 0) return;
  int nblk;
  const int64_t chunk = def_chunk(P, &nblk);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_rows_diff_sqnorm, dim3(nblk, (unsigned)ceil_div(C, kDefRows)), dim3(kDefThreads), 0, st,
                     ptr<const float>(rows), ptr<const float>(ref), (int)C, P, stride, chunk, ptr<double>(part), nblk);
  hipLaunchKernelGGL(k_rows_norm_finish, dim3((unsigned)C), dim3(kDefThreads), 0, st, ptr<const double>(part), nblk,
                     ptr<float>(norm));
  NIDT_CHECK(hipGetLastError());
}

// One coordinate of one row: d = v - g; r = d / m + g; r = r + stddev * z; acc = fma(w, r, acc) - the operation order
// the torch twin in engine/defense.py follows (r + stddev * z rounds twice: contraction is off).
template <bool NOISE>
__device__ __forceinline__ float clip_term(float v, float g, float m, float w, float acc, bool noisy, float stddev,
                                           uint64_t seed, uint32_t cid, uint32_t j) {
#pragma clang fp contract(off)
  const float d = v - g;
  float r = (m == 1.f ? d : __fdiv_rn(d, m)) + g;  // d / 1 == d: unclipped rows skip the division
  if (NOISE) {
    if (noisy) r = r + stddev * noise_z(seed, cid, j);
  }
  return fmaf(w, r, acc);
}

// One thread per 4 coordinates, rows in ascending order (k_weighted_rows_sum's shape; the last P % 4 coordinates are
// one thread's scalar tail).  The per-row scale m_c = max(1, norm[c] / bound), weight and client id are staged
// through LDS once per block (kDefThreads rows at a time), so the division by the bound is not repeated per
// coordinate.
template <bool NOISE>
__global__ __launch_bounds__(kDefThreads) void k_clipped_rows_sum(
    const float* __restrict__ rows, const float* __restrict__ ref, const float* __restrict__ wts,
    const float* __restrict__ norm, const int* __restrict__ cids, int C, int64_t P, int64_t stride, float norm_bound,
    float stddev, uint64_t seed, const uint32_t* __restrict__ mbits, float* __restrict__ out) {
  __shared__ float s_m[kDefThreads], s_w[kDefThreads];
  __shared__ uint32_t s_id[kDefThreads];
  const int64_t i = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  const bool vec = i + 3 < P;
  const int nt = (vec || i >= P) ? 0 : (int)(P - i);  // 1..3 coordinates of the thread that owns the row tail
  const uint32_t j0 = (uint32_t)i;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f), acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    g = *reinterpret_cast<const float4*>(ref + i);
  } else if (nt) {
    g.x = ref[i];
    if (nt > 1) g.y = ref[i + 1];
    if (nt > 2) g.z = ref[i + 2];
  }
  uint32_t nib = 0xfu;  // noise only where the shared mask keeps the coordinate
  if (NOISE && mbits != nullptr && (vec || nt)) nib = (mbits[i >> 5] >> (i & 31)) & 0xfu;
  for (int c0 = 0; c0 < C; c0 += kDefThreads) {
    const int n = C - c0 < kDefThreads ? C - c0 : kDefThreads;
    __syncthreads();
    if ((int)threadIdx.x < n) {
      s_m[threadIdx.x] = fmaxf(1.f, __fdiv_rn(norm[c0 + threadIdx.x], norm_bound));
      s_w[threadIdx.x] = wts[c0 + threadIdx.x];
      s_id[threadIdx.x] = NOISE ? (uint32_t)cids[c0 + threadIdx.x] : 0u;
    }
    __syncthreads();
    if (vec) {
      const float* row = rows + (int64_t)c0 * stride + i;
      for (int k = 0; k < n; ++k, row += stride) {
        const float m = s_m[k], w = s_w[k];
        const uint32_t id = s_id[k];
        const float4 v = *reinterpret_cast<const float4*>(row);
        acc.x = clip_term<NOISE>(v.x, g.x, m, w, acc.x, nib & 1u, stddev, seed, id, j0);
        acc.y = clip_term<NOISE>(v.y, g.y, m, w, acc.y, nib & 2u, stddev, seed, id, j0 + 1u);
        acc.z = clip_term<NOISE>(v.z, g.z, m, w, acc.z, nib & 4u, stddev, seed, id, j0 + 2u);
        acc.w = clip_term<NOISE>(v.w, g.w, m, w, acc.w, nib & 8u, stddev, seed, id, j0 + 3u);
      }
    } else if (nt) {
      const float* row = rows + (int64_t)c0 * stride + i;
      for (int k = 0; k < n; ++k, row += stride) {
        const float m = s_m[k], w = s_w[k];
        const uint32_t id = s_id[k];
        acc.x = clip_term<NOISE>(row[0], g.x, m, w, acc.x, nib & 1u, stddev, seed, id, j0);
        if (nt > 1) acc.y = clip_term<NOISE>(row[1], g.y, m, w, acc.y, nib & 2u, stddev, seed, id, j0 + 1u);
        if (nt > 2) acc.z = clip_term<NOISE>(row[2], g.z, m, w, acc.z, nib & 4u, stddev, seed, id, j0 + 2u);
      }
    }
  }
  if (vec) {
    *reinterpret_cast<float4*>(out + i) = acc;
  } else if (nt) {
    out[i] = acc.x;
    if (nt > 1) out[i + 1] = acc.y;
    if (nt > 2) out[i + 2] = acc.z;
  }
}

void clipped_rows_sum(uintptr_t rows, uintptr_t ref, uintptr_t wts, uintptr_t norm, uintptr_t cids, int64_t C,
                      int64_t P, int64_t stride, float norm_bound, float stddev, uint64_t seed, uintptr_t mbits,
                      uintptr_t out, uintptr_t stream) {
  NIDT_REQUIRE(stride % 4 == 0 && stride >= P && (rows & 15) == 0 && (ref & 15) == 0 && (out & 15) == 0,
               "clipped_rows_sum: 16-byte aligned rows, ref and out (stride % 4 == 0, stride >= P)");
  NIDT_REQUIRE(C >= 0 && P >= 0 && P < (int64_t(1) << 32) && rows != 0 && ref != 0 && wts != 0 && norm != 0 &&
                   out != 0 && norm_bound > 0.f && stddev >= 0.f && (stddev == 0.f || cids != 0),
               "clipped_rows_sum: arguments (norm_bound > 0, stddev >= 0, client ids with stddev > 0)");
  if (P == 0) return;
  const int64_t n4 = (P + 3) / 4;
  const dim3 grid(ceil_div(n4, kDefThreads));
  if (stddev > 0.f)
    hipLaunchKernelGGL(k_clipped_rows_sum<true>, grid, dim3(kDefThreads), 0, as_stream(stream), ptr<const float>(rows),
                       ptr<const float>(ref), ptr<const float>(wts), ptr<const float>(norm), ptr<const int>(cids),
                       (int)C, P, stride, norm_bound, stddev, seed, ptr<const uint32_t>(mbits), ptr<float>(out));
  else
    hipLaunchKernelGGL(k_clipped_rows_sum<false>, grid, dim3(kDefThreads), 0, as_stream(stream),
                       ptr<const float>(rows), ptr<const float>(ref), ptr<const float>(wts), ptr<const float>(norm),
                       ptr<const int>(cids), (int)C, P, stride, norm_bound, stddev, seed, ptr<const uint32_t>(mbits),
                       ptr<float>(out));
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
