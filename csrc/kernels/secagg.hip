// Secure aggregation (masked FedAvg over Z_p, p = 2^31 - 1) on the client rows.  One protocol definition serves
// these kernels, the numpy twins (engine/secagg.py) and the host trainer (algorithms/turboaggregate.py,
// TurboAggregateTrainer(prg="counter")):
//
//   q_i[j]  = rint((double(theta_i[j]) * w_i) * S), |q| saturated at B, non-finite -> 0          (fixed point in Z_p)
//   m(key, round, seg, j) = z mod p, z = the 64-bit splitmix finaliser over seed = (round << 32) | key, a = seg, b = j
//   upload_i[j] = q_i[j] + sum_{peers k} (k > i ? m(key_ik) : p - m(key_ik))   (mod p)
//
//   secagg_upload     : the C masked rows, uint32 [C, P] in [0, p): what each client would send
//   secagg_masked_sum : the column sum of those rows mod p without materialising them, as int64 [P]; the caller lists
//                       per row only the peers whose masks do not cancel inside the launch
//   secagg_finish     : the reduced int64 [P] minus the survivors' masks towards dropped clients, mod p, centred,
//                       float32(double(c) / S / a)
//
// rows is the [*, ld] fp32 client matrix read in place through a row list (16-B aligned rows; rows that are not
// listed and the pad columns [P, ld) are never read); nothing is written past P of an output.  Integer arithmetic in
// plain C++, vector stores, no atomics: every output is a function of (row contents, keys) only, so the aggregate is
// bit-identical for any sharding of the clients.  z mod p is a Mersenne fold (2^31 = 1 mod p), exact for every z.
//
// The masks are a statistical PRG, as the reference's numpy streams are: this simulates the protocol's data flow and
// cost and makes no cryptographic strength claim.
#include "common.h"

namespace nidt {

constexpr int kSecThreads = 256;
constexpr uint32_t kSecP = 0x7fffffffu;  // 2^31 - 1

// every bit of the splitmix finaliser whose high half is def_mix_hash / mix_hash (numpy twin: _mix_hash64_np)
__device__ __forceinline__ uint64_t sec_mix64(uint64_t seed, uint32_t a, uint32_t b) {
  uint64_t z = seed ^ (0x9e3779b97f4a7c15ull * (((uint64_t)a << 32) ^ (uint64_t)b));
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

// z mod (2^31 - 1): z = t * 2^62 + h * 2^31 + l = t + h + l (mod p).  The sum reaches 2p + 3 = 2^32 + 1, one bit more
// than 32, so it is formed in 64 bits; it folds once more to <= p + 2 and one conditional subtraction finishes.
__device__ __forceinline__ uint32_t sec_modp(uint64_t z) {
  const uint64_t t = (z & kSecP) + ((z >> 31) & kSecP) + (z >> 62);  // <= 2p + 3
  uint32_t s = (uint32_t)(t & kSecP) + (uint32_t)(t >> 31);          // <= p + 2
  s = s >= kSecP ? s - kSecP : s;
  return s;
}

__device__ __forceinline__ uint32_t sec_mask(uint64_t seed, uint32_t seg, uint32_t j) {
  return sec_modp(sec_mix64(seed, seg, j));
}

// Fixed point of one coordinate as a residue in [0, p); *bad counts saturated and non-finite values.
__device__ __forceinline__ uint32_t sec_quant(float v, double w, double S, double B, int* bad) {
#pragma clang fp contract(off)
  const double x = ((double)v * w) * S;
  double r = rint(x);  // round half to even
  if (!(fabs(x) <= 1.7976931348623157e308)) {  // NaN or Inf
    r = 0.0;
    ++*bad;
  } else if (r > B) {
    r = B;
    ++*bad;
  } else if (r < -B) {
    r = -B;
    ++*bad;
  }
  const int32_t q = (int32_t)r;  // |r| <= B < 2^30
  return q < 0 ? (uint32_t)(q + (int32_t)kSecP) : (uint32_t)q;
}

// One row's 1 .. 4 coordinates from column i: quantised value plus the row's listed pair masks, each lane a sum of
// residues (< npeer * p + p: a uint64 holds it for any list).
__device__ __forceinline__ void sec_row_terms(const float* __restrict__ row, int64_t i, int nv, bool vec, double w,
                                              double S, double B, int cid, const int* __restrict__ pid,
                                              const int* __restrict__ pkey, int np, uint64_t round_hi, uint32_t seg,
                                              uint64_t acc[4], int* bad) {
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(row + i);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    for (int u = 0; u < nv; ++u) v[u] = row[i + u];
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (u < nv) acc[u] += sec_quant(v[u], w, S, B, bad);
  const uint32_t j0 = (uint32_t)i;
  for (int k = 0; k < np; ++k) {  // wave-uniform list entries
    const uint64_t seed = round_hi | (uint64_t)(uint32_t)pkey[k];
    const bool neg = pid[k] < cid;  // the lower id of a pair adds m, the higher p - m
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (u < nv) {
        const uint32_t m = sec_mask(seed, seg, j0 + (uint32_t)u);
        acc[u] += neg ? kSecP - m : m;
      }
    }
  }
}

// block reduction of the per-thread counts into cnt[block] (every block writes its slot)
__device__ __forceinline__ void sec_block_count(int bad, int* __restrict__ cnt, int slot) {
  __shared__ int red[kSecThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kSecThreads / 64; ++w) t += red[w];
    cnt[slot] = t;
  }
}

// grid (ceil(P / 4 / 256), C): thread = 4 columns of one listed row.
__global__ __launch_bounds__(kSecThreads) void k_secagg_upload(
    const float* __restrict__ rows, int64_t stride, const int* __restrict__ ridx, const int* __restrict__ cids,
    const double* __restrict__ wts, const int* __restrict__ poff, const int* __restrict__ pid,
    const int* __restrict__ pkey, int64_t P, uint64_t round_hi, uint32_t seg, double S, double B,
    uint32_t* __restrict__ out, int* __restrict__ cnt) {
  const int c = blockIdx.y;
  const int64_t i = 4 * ((int64_t)blockIdx.x * kSecThreads + threadIdx.x);
  const int nv = i >= P ? 0 : (P - i < 4 ? (int)(P - i) : 4);
  int bad = 0;
  if (nv) {
    uint64_t acc[4] = {0, 0, 0, 0};
    const int p0 = poff[c];
    sec_row_terms(rows + (int64_t)ridx[c] * stride, i, nv, nv == 4, wts[c], S, B, cids[c], pid + p0, pkey + p0,
                  poff[c + 1] - p0, round_hi, seg, acc, &bad);
    uint32_t* o = out + (int64_t)c * P + i;  // rows of P words: 4-B aligned only
    for (int u = 0; u < nv; ++u) o[u] = sec_modp(acc[u]);
  }
  sec_block_count(bad, cnt, blockIdx.y * gridDim.x + blockIdx.x);
}

// grid (ceil(P / 4 / 256)): thread = 4 columns, the listed rows in list order.
__global__ __launch_bounds__(kSecThreads) void k_secagg_masked_sum(
    const float* __restrict__ rows, int64_t stride, const int* __restrict__ ridx, const int* __restrict__ cids,
    const double* __restrict__ wts, const int* __restrict__ poff, const int* __restrict__ pid,
    const int* __restrict__ pkey, int C, int64_t P, uint64_t round_hi, uint32_t seg, double S, double B,
    int64_t* __restrict__ out, int* __restrict__ cnt) {
  const int64_t i = 4 * ((int64_t)blockIdx.x * kSecThreads + threadIdx.x);
  const int nv = i >= P ? 0 : (P - i < 4 ? (int)(P - i) : 4);
  int bad = 0;
  if (nv) {
    uint64_t acc[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
      const int p0 = poff[c];
      sec_row_terms(rows + (int64_t)ridx[c] * stride, i, nv, nv == 4, wts[c], S, B, cids[c], pid + p0, pkey + p0,
                    poff[c + 1] - p0, round_hi, seg, acc, &bad);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = sec_modp(acc[u]);  // keeps the lanes far from 2^64 for any C
    }
    if (nv == 4) {  // out is 16-B aligned
      longlong2* o = reinterpret_cast<longlong2*>(out + i);
      o[0] = make_longlong2((long long)acc[0], (long long)acc[1]);
      o[1] = make_longlong2((long long)acc[2], (long long)acc[3]);
    } else {
      for (int u = 0; u < nv; ++u) out[i + u] = (int64_t)acc[u];
    }
  }
  sec_block_count(bad, cnt, blockIdx.x);
}

// grid (ceil(P / 4 / 256)): thread = 4 columns.  sum[j] is a sum of residues (of the ranks' partials), read as an
// unsigned 64-bit value; the npair
// (survivor, dropped, key) entries name the masks the survivors added towards clients that never uploaded.
__global__ __launch_bounds__(kSecThreads) void k_secagg_finish(
    const int64_t* __restrict__ sum, int64_t P, const int* __restrict__ sid, const int* __restrict__ did,
    const int* __restrict__ pkey, int npair, uint64_t round_hi, uint32_t seg, double S, double a,
    float* __restrict__ out) {
  const int64_t i = 4 * ((int64_t)blockIdx.x * kSecThreads + threadIdx.x);
  const int nv = i >= P ? 0 : (P - i < 4 ? (int)(P - i) : 4);
  if (!nv) return;
  uint64_t acc[4] = {0, 0, 0, 0};
  for (int u = 0; u < nv; ++u) acc[u] = sec_modp((uint64_t)sum[i + u]);
  const uint32_t j0 = (uint32_t)i;
  for (int k = 0; k < npair; ++k) {
    const uint64_t seed = round_hi | (uint64_t)(uint32_t)pkey[k];
    const bool added_neg = did[k] < sid[k];  // the survivor added p - m: take it back by adding m
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (u < nv) {
        const uint32_t m = sec_mask(seed, seg, j0 + (uint32_t)u);
        acc[u] += added_neg ? m : kSecP - m;
      }
    }
    if ((k & 1023) == 1023) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = sec_modp(acc[u]);
    }
  }
  for (int u = 0; u < nv; ++u) {
#pragma clang fp contract(off)
    const uint32_t s = sec_modp(acc[u]);
    const int32_t c = s > (kSecP >> 1) ? (int32_t)s - (int32_t)kSecP : (int32_t)s;  // (-p/2, p/2]
    out[i + u] = (float)(((double)c / S) / a);
  }
}

int64_t secagg_blocks(int64_t P) { return P > 0 ? ((P + 3) / 4 + kSecThreads - 1) / kSecThreads : 1; }

static void sec_check_rows(uintptr_t rows, int64_t stride, int64_t C, int64_t P, int64_t round, int64_t seg,
                           double S, double B, const char* what) {
  NIDT_REQUIRE(rows != 0 && (rows & 15) == 0 && stride % 4 == 0 && stride >= P, what);
  NIDT_REQUIRE(C >= 1 && C <= 65535 && P >= 1 && P < (int64_t(1) << 32), what);
  NIDT_REQUIRE(round >= 0 && round < (int64_t(1) << 32) && (seg == 0 || seg == 1), what);
  NIDT_REQUIRE(S >= 1.0 && B >= 1.0 && B <= 1073741823.0, what);
}

void secagg_upload(uintptr_t rows, int64_t stride, uintptr_t ridx, uintptr_t cids, uintptr_t wts, uintptr_t poff,
                   uintptr_t pid, uintptr_t pkey, int64_t C, int64_t P, int64_t round, int64_t seg, double S, double B,
                   uintptr_t out, uintptr_t cnt, uintptr_t stream) {
  sec_check_rows(rows, stride, C, P, round, seg, S, B,
                 "secagg_upload: 16-byte aligned fp32 rows (stride % 4 == 0, stride >= P), 1 <= C <= 65535, "
                 "1 <= P < 2^32, 0 <= round < 2^32, seg 0 | 1, S >= 1, 1 <= B < 2^30");
  NIDT_REQUIRE(ridx && cids && wts && poff && out && cnt && (wts & 7) == 0 && (out & 3) == 0,
               "secagg_upload: null or misaligned argument");
  hipLaunchKernelGGL(k_secagg_upload, dim3((unsigned)secagg_blocks(P), (unsigned)C), dim3(kSecThreads), 0,
                     as_stream(stream), ptr<const float>(rows), stride, ptr<const int>(ridx), ptr<const int>(cids),
                     ptr<const double>(wts), ptr<const int>(poff), ptr<const int>(pid), ptr<const int>(pkey), P,
                     (uint64_t)round << 32, (uint32_t)seg, S, B, ptr<uint32_t>(out), ptr<int>(cnt));
  NIDT_CHECK(hipGetLastError());
}

void secagg_masked_sum(uintptr_t rows, int64_t stride, uintptr_t ridx, uintptr_t cids, uintptr_t wts, uintptr_t poff,
                       uintptr_t pid, uintptr_t pkey, int64_t C, int64_t P, int64_t round, int64_t seg, double S,
                       double B, uintptr_t out, uintptr_t cnt, uintptr_t stream) {
  sec_check_rows(rows, stride, C, P, round, seg, S, B,
                 "secagg_masked_sum: 16-byte aligned fp32 rows (stride % 4 == 0, stride >= P), 1 <= C <= 65535, "
                 "1 <= P < 2^32, 0 <= round < 2^32, seg 0 | 1, S >= 1, 1 <= B < 2^30");
  NIDT_REQUIRE(ridx && cids && wts && poff && out && cnt && (wts & 7) == 0 && (out & 15) == 0,
               "secagg_masked_sum: null or misaligned argument (16-byte aligned int64 out)");
  hipLaunchKernelGGL(k_secagg_masked_sum, dim3((unsigned)secagg_blocks(P)), dim3(kSecThreads), 0, as_stream(stream),
                     ptr<const float>(rows), stride, ptr<const int>(ridx), ptr<const int>(cids),
                     ptr<const double>(wts), ptr<const int>(poff), ptr<const int>(pid), ptr<const int>(pkey), (int)C,
                     P, (uint64_t)round << 32, (uint32_t)seg, S, B, ptr<int64_t>(out), ptr<int>(cnt));
  NIDT_CHECK(hipGetLastError());
}

void secagg_finish(uintptr_t sum, int64_t P, uintptr_t sid, uintptr_t did, uintptr_t pkey, int64_t npair,
                   int64_t round, int64_t seg, double S, double a, uintptr_t out, uintptr_t stream) {
  NIDT_REQUIRE(sum != 0 && (sum & 7) == 0 && out != 0 && (out & 3) == 0 && P >= 1 && P < (int64_t(1) << 32),
               "secagg_finish: int64 sum and fp32 out, 1 <= P < 2^32");
  NIDT_REQUIRE(npair >= 0 && npair < (int64_t(1) << 31) && (npair == 0 || (sid && did && pkey)),
               "secagg_finish: the pair list");
  NIDT_REQUIRE(round >= 0 && round < (int64_t(1) << 32) && (seg == 0 || seg == 1) && S >= 1.0 && a > 0.0 && a <= 1.0,
               "secagg_finish: 0 <= round < 2^32, seg 0 | 1, S >= 1, 0 < a <= 1");
  hipLaunchKernelGGL(k_secagg_finish, dim3((unsigned)secagg_blocks(P)), dim3(kSecThreads), 0, as_stream(stream),
                     ptr<const int64_t>(sum), P, ptr<const int>(sid), ptr<const int>(did), ptr<const int>(pkey),
                     (int)npair, (uint64_t)round << 32, (uint32_t)seg, S, a, ptr<float>(out));
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
