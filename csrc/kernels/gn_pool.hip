// GroupNorm + ReLU + 2x2 max-pool of the client-batched 2-D zoo (vgg11 / vgg16: GroupNorm(32, C), ReLU, MaxPool2d(2, 2)
// between two bf16 convs) as one forward and one backward kernel over channels-last bf16 activations
// t [N = G*B][H][W][C], and the plain 2x2 stride-2 max-pool of the models that pool without a GroupNorm.
//
// Unit of work: one 8-channel chunk column x one 2x2 window (four 16-B chunks; one chunk without the pool).  The four
// window positions live in one thread, so the pool, its argmax and the routing of the gradient are register-local and
// only the pooled chunk is stored; neither a mask nor an index tensor exists (the backward recomputes both from t and
// the saved statistics with the forward's own arithmetic: sc = gamma rstd, sh = beta - mean sc, z = fma(t, sc, sh),
// the first maximum of a window in (row, column) order takes the gradient).
//
// A block of 512 threads takes as many whole samples of ONE client as fill it: a sample of U units gets
// tps = min(512, pow2ceil(U)) threads (a "slot"), a block holds spb = 512 / tps slots, a client's B samples take
// ceil(B / spb) blocks and the ragged last one is masked (the buffer range ends at the client's last sample, so loads
// past it read zeros and stores are dropped).  Samples of more than 512 units give each thread NU = 2 .. 16 units,
// 512 apart.  tps and 512 are multiples of C / 8, so a thread's chunk column is fixed for the whole kernel.
// The sample is read from HBM once and held packed (<= 16 chunks per thread); statistics are two-pass from the
// registers.  Reductions: xor shuffles over the lanes of a slot that share a column, then the slot's wave segments
// and the channels of a group through LDS in a fixed order: no atomics, bit-reproducible.
#include "common.h"
#include "dma.h"

namespace nidt {

constexpr int kGpThreads = 512;

__device__ __forceinline__ void gp_unpack8(const i32x4_t v, float* f) {
  const uint32_t u[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(u[j] << 16);
    f[2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
  }
}

__device__ __forceinline__ i32x4_t gp_pack8(const float* f) {
  i32x4_t o;
  o.x = (int)pack_bf16x2(f[0], f[1]);
  o.y = (int)pack_bf16x2(f[2], f[3]);
  o.z = (int)pack_bf16x2(f[4], f[5]);
  o.w = (int)pack_bf16x2(f[6], f[7]);
  return o;
}

// The held chunks are redefined opaquely between passes, so that a pass's unpacked fp32 copies do not stay live.
template <int NV>
__device__ __forceinline__ void gp_fence(i32x4_t (&v)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) asm volatile("" : "+v"(v[k]));
}

// How a launch splits the samples (the launcher's plan, passed by value).
struct GpPlan {
  int B, H, W, C, groups;
  int lnch, lcg;      // log2 of the chunk columns C / 8 and of the channels per group
  int U;              // units per sample
  int tps, ltps;      // threads per sample slot (a power of two, >= C / 8), its log2
  int spb, bpc;       // slots per block, blocks per client
  int nred, nchs;     // LDS floats: the segment partials (512 / seg) * C and the per-slot channel sums spb * C
};

// Per-(slot, channel) totals of every thread's 8 channel partials p (channels 8j .. 8j+7 of its column j): the lanes
// of a segment (seg = min(tps, 64) consecutive lanes of one slot) that share j by xor shuffles, then the slot's
// segments in a fixed order through LDS.  red: LDS [512 / seg][C]; out: LDS [spb][C] (valid after the call).
__device__ __forceinline__ void gp_chan_sums(float* p, float* red, float* out, const GpPlan& g) {
  const int tid = threadIdx.x, nch = 1 << g.lnch, C = g.C;
  const int lseg = g.ltps < 6 ? g.ltps : 6, seg = 1 << lseg;
  for (int o = nch; o < seg; o <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] += __shfl_xor(p[e], o, 64);
  if ((tid & (seg - 1)) < nch) {
    float4* r = reinterpret_cast<float4*>(red + (tid >> lseg) * C + 8 * (tid & (nch - 1)));
    r[0] = make_float4(p[0], p[1], p[2], p[3]);
    r[1] = make_float4(p[4], p[5], p[6], p[7]);
  }
  __syncthreads();
  const int sps = g.tps >> lseg;  // segments per slot
  for (int i = tid; i < g.nchs; i += kGpThreads) {
    const int s = i / C, c = i - s * C;
    float a = 0.f;
    for (int q = 0; q < sps; ++q) a += red[(s * sps + q) * C + c];
    out[i] = a;
  }
  __syncthreads();
}

// The byte offset of unit k's output chunk (pooled with POOL; without it the input chunk is the same one) inside the
// block's buffer range; kBufOOB for a unit that does not exist: a thread past the sample's units or a slot past the
// client's samples.
template <bool POOL>
__device__ __forceinline__ int gp_out(const GpPlan& g, int k, int ns) {
  const int tid = threadIdx.x, slot = tid >> g.ltps, u = (tid & (g.tps - 1)) + k * g.tps;
  const int So = POOL ? (g.H * g.W) >> 2 : g.H * g.W;
  return (u < g.U && slot < ns) ? slot * So * g.C * 2 + u * 16 : kBufOOB;
}

// The byte offset of the first chunk of pooled unit k's window (kept in a register: it takes a division).
__device__ __forceinline__ int gp_in(const GpPlan& g, int k, int ns) {
  const int tid = threadIdx.x, slot = tid >> g.ltps, u = (tid & (g.tps - 1)) + k * g.tps;
  const int Wo = g.W >> 1, p = u >> g.lnch, ho = p / Wo, wo = p - ho * Wo;
  return (u < g.U && slot < ns)
             ? (slot * g.H * g.W + 2 * ho * g.W + 2 * wo) * g.C * 2 + (tid & ((1 << g.lnch) - 1)) * 16 : kBufOOB;
}

// Chunk i (0 .. 3: (row, column) order of the window) of a unit, in bytes past the unit's first chunk.
__device__ __forceinline__ int gp_win(const GpPlan& g, int i) { return ((i >> 1) * g.W + (i & 1)) * g.C * 2; }

template <int NU, bool POOL, bool RELU>
__global__ __launch_bounds__(kGpThreads, 4) void k_gn2d_fwd(const uint16_t* __restrict__ t,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int64_t ld,
                                                            uint16_t* __restrict__ y, float* __restrict__ stats,
                                                            float eps, const GpPlan g) {
  constexpr int CPU = POOL ? 4 : 1, NC = NU * CPU;
  extern __shared__ __attribute__((aligned(16))) float gp_lds[];
  float* red = gp_lds;
  float* chs = gp_lds + g.nred;
  const int tid = threadIdx.x, C = g.C, S = g.H * g.W, cg = 1 << g.lcg;
  const int cl = blockIdx.x / g.bpc, b0 = (blockIdx.x - cl * g.bpc) * g.spb;
  const int ns = min(g.spb, g.B - b0);  // samples of this block (the client's ragged last block: fewer)
  const int64_t n0 = (int64_t)cl * g.B + b0;
  const int slot = tid >> g.ltps, j = tid & ((1 << g.lnch) - 1);
  const i32x4_t rt = make_rsrc(t + n0 * S * C, (uint32_t)ns * S * C * 2);
  const i32x4_t ry = make_rsrc(y + n0 * (POOL ? S >> 2 : S) * C, (uint32_t)ns * (POOL ? S >> 2 : S) * C * 2);
  int uo[POOL ? NU : 1];
  auto in_off = [&](int k) { return POOL ? uo[k] : gp_out<false>(g, k, ns); };
  i32x4_t v[NC];
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    if (POOL) uo[k] = gp_in(g, k, ns);
#pragma unroll
    for (int i = 0; i < CPU; ++i)
      v[k * CPU + i] = nidt_raw_buffer_load_v4i32(rt, in_off(k) + (POOL ? gp_win(g, i) : 0), 0, 0);
  }
  float part[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) part[e] = 0.f;
#pragma unroll
  for (int q = 0; q < NC; ++q) {  // units that do not exist read zeros: no guard in the sum
    float f[8];
    gp_unpack8(v[q], f);
#pragma unroll
    for (int e = 0; e < 8; ++e) part[e] += f[e];
  }
  gp_chan_sums(part, red, chs, g);
  const int npair = g.spb * g.groups;  // (slot, group); <= nred
  for (int i = tid; i < npair; i += kGpThreads) {
    const int s = i / g.groups, gi = i - s * g.groups;
    float a = 0.f;
    for (int q = 0; q < cg; ++q) a += chs[s * C + gi * cg + q];
    const float m = a / (float)(S * cg);
    red[i] = m;
    if (stats && s < ns) stats[((n0 + s) * g.groups + gi) * 2] = m;
  }
  __syncthreads();
  gp_fence(v);
  float mu[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mu[e] = red[slot * g.groups + ((8 * j + e) >> g.lcg)];
    part[e] = 0.f;
  }
  __syncthreads();  // red is written again below
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    if (in_off(k) >= 0) {
#pragma unroll
      for (int i = 0; i < CPU; ++i) {
        float f[8];
        gp_unpack8(v[k * CPU + i], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = f[e] - mu[e];
          part[e] = fmaf(d, d, part[e]);
        }
      }
    }
  }
  gp_chan_sums(part, red, chs, g);
  for (int i = tid; i < npair; i += kGpThreads) {
    const int s = i / g.groups, gi = i - s * g.groups;
    float a = 0.f;
    for (int q = 0; q < cg; ++q) a += chs[s * C + gi * cg + q];
    const float rs = rsqrtf(a / (float)(S * cg) + eps);
    red[i] = rs;
    if (stats && s < ns) stats[((n0 + s) * g.groups + gi) * 2 + 1] = rs;
  }
  __syncthreads();
  float sc[8], sh[8];
  const float* gw = gamma + (int64_t)cl * ld;
  const float* gb = beta + (int64_t)cl * ld;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = 8 * j + e;
    sc[e] = gw[c] * red[slot * g.groups + (c >> g.lcg)];
    sh[e] = gb[c] - mu[e] * sc[e];
  }
  gp_fence(v);
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    float a[8];
#pragma unroll
    for (int i = 0; i < CPU; ++i) {
      float f[8];
      gp_unpack8(v[k * CPU + i], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float z = fmaf(f[e], sc[e], sh[e]);
        a[e] = (i == 0 || z > a[e]) ? z : a[e];
      }
    }
    if (RELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = fmaxf(a[e], 0.f);
    }
    nidt_raw_buffer_store_v4i32(gp_pack8(a), ry, gp_out<POOL>(g, k, ns), 0, 0);  // units that do not exist: dropped
  }
}

// dy: bf16 in the shape of y; dt: bf16 in the shape of t; part_out [N][C][2] = (dbeta, dgamma) per sample.
// t and dy are read once and held packed; the first pass finds each window's first maximum and ReLU mask, replaces
// the held dy by the masked one and keeps the winners as 2 bits per channel.
template <int NU, bool POOL, bool RELU>
__global__ __launch_bounds__(kGpThreads, (POOL ? NU * 5 : NU * 2) > 8 ? 2 : 4) void k_gn2d_bwd(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ t, const float* __restrict__ stats,
    const float* __restrict__ gamma, const float* __restrict__ beta, int64_t ld, uint16_t* __restrict__ dt,
    float* __restrict__ part_out, const GpPlan g) {
  constexpr int CPU = POOL ? 4 : 1, NC = NU * CPU;
  extern __shared__ __attribute__((aligned(16))) float gp_lds[];
  float* red = gp_lds;  // then the group means of dy gamma xhat
  float* chA = gp_lds + g.nred;
  float* chB = chA + g.nchs;
  float* gm1 = chB + g.nchs;  // [spb][groups]
  const int tid = threadIdx.x, C = g.C, S = g.H * g.W, cg = 1 << g.lcg;
  const int cl = blockIdx.x / g.bpc, b0 = (blockIdx.x - cl * g.bpc) * g.spb;
  const int ns = min(g.spb, g.B - b0);
  const int64_t n0 = (int64_t)cl * g.B + b0;
  const int slot = tid >> g.ltps, j = tid & ((1 << g.lnch) - 1);
  const int64_t ns_ = n0 + min(slot, ns - 1);  // a slot past the client's samples reads the last one's statistics
  const float* gw_ = gamma + (int64_t)cl * ld;
  float mu[8], rs[8], gw[8], msc[8], msh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = 8 * j + e;
    mu[e] = stats[(ns_ * g.groups + (c >> g.lcg)) * 2];
    rs[e] = stats[(ns_ * g.groups + (c >> g.lcg)) * 2 + 1];
    gw[e] = gw_[c];
    if (POOL || RELU) {  // k_gn2d_fwd's coefficients, same expressions
      msc[e] = gw[e] * rs[e];
      msh[e] = beta[(int64_t)cl * ld + c] - mu[e] * msc[e];
    }
  }
  const i32x4_t rt = make_rsrc(t + n0 * S * C, (uint32_t)ns * S * C * 2);
  const i32x4_t rdt = make_rsrc(dt + n0 * S * C, (uint32_t)ns * S * C * 2);
  const i32x4_t rd = make_rsrc(dy + n0 * (POOL ? S >> 2 : S) * C, (uint32_t)ns * (POOL ? S >> 2 : S) * C * 2);
  int uo[POOL ? NU : 1];
  auto in_off = [&](int k) { return POOL ? uo[k] : gp_out<false>(g, k, ns); };
  uint32_t sel[POOL ? NU : 1];
  i32x4_t v[NC], dv[NU];
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    if (POOL) uo[k] = gp_in(g, k, ns);
#pragma unroll
    for (int i = 0; i < CPU; ++i)
      v[k * CPU + i] = nidt_raw_buffer_load_v4i32(rt, in_off(k) + (POOL ? gp_win(g, i) : 0), 0, 0);
    dv[k] = nidt_raw_buffer_load_v4i32(rd, gp_out<POOL>(g, k, ns), 0, 0);
  }
  float pa[8], pb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) pa[e] = pb[e] = 0.f;
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    float d[8], zb[8], xb[8];
    gp_unpack8(dv[k], d);
    uint32_t w = 0;  // the window's winners, 2 bits per channel
#pragma unroll
    for (int i = 0; i < CPU; ++i) {
      float f[8];
      gp_unpack8(v[k * CPU + i], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float z = (POOL || RELU) ? fmaf(f[e], msc[e], msh[e]) : 0.f;
        if (i == 0 || z > zb[e]) {  // strictly greater: the first maximum keeps the gradient
          zb[e] = z;
          xb[e] = f[e];
          if (i) w = (w & ~(3u << (2 * e))) | ((uint32_t)i << (2 * e));
        }
      }
    }
    if (POOL) sel[k] = w;
    if (RELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = zb[e] > 0.f ? d[e] : 0.f;
      dv[k] = gp_pack8(d);  // exact: bf16 values or zero
    }
    if (in_off(k) >= 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pa[e] += d[e];
        pb[e] = fmaf(d[e], (xb[e] - mu[e]) * rs[e], pb[e]);
      }
    }
  }
  // per-channel A_c (= dbeta partial) and B_c (= dgamma partial), then the group means of the gamma-weighted sums
  gp_chan_sums(pa, red, chA, g);
  gp_chan_sums(pb, red, chB, g);
  for (int i = tid; i < g.nchs; i += kGpThreads) {
    const int s = i / C, c = i - s * C;
    if (s < ns) {
      part_out[((n0 + s) * C + c) * 2] = chA[i];
      part_out[((n0 + s) * C + c) * 2 + 1] = chB[i];
    }
  }
  for (int i = tid; i < g.spb * g.groups; i += kGpThreads) {
    const int s = i / g.groups, gi = i - s * g.groups;
    float s1 = 0.f, s2 = 0.f;
    for (int q = 0; q < cg; ++q) {
      const int c = gi * cg + q;
      s1 = fmaf(gw_[c], chA[s * C + c], s1);
      s2 = fmaf(gw_[c], chB[s * C + c], s2);
    }
    gm1[i] = s1 / (float)(S * cg);
    red[i] = s2 / (float)(S * cg);
  }
  __syncthreads();
  float m1[8], m2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m1[e] = gm1[slot * g.groups + ((8 * j + e) >> g.lcg)];
    m2[e] = red[slot * g.groups + ((8 * j + e) >> g.lcg)];
  }
  gp_fence(v);
  gp_fence(dv);
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    float d[8];
    gp_unpack8(dv[k], d);
#pragma unroll
    for (int i = 0; i < CPU; ++i) {
      float f[8], r[8];
      gp_unpack8(v[k * CPU + i], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float dd = (!POOL || ((sel[POOL ? k : 0] >> (2 * e)) & 3u) == (uint32_t)i) ? d[e] : 0.f;
        const float x = (f[e] - mu[e]) * rs[e];
        r[e] = rs[e] * (dd * gw[e] - m1[e] - x * m2[e]);
      }
      nidt_raw_buffer_store_v4i32(gp_pack8(r), rdt, in_off(k) + (POOL ? gp_win(g, i) : 0), 0, 0);
    }
  }
}

static bool gp_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static int gp_log2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// The served shapes (conv2d_hip.gn2d_ok mirrors this rule) and the split of a launch.
static GpPlan gp_plan(int N, int B, int H, int W, int C, int groups, int pool, const char* who) {
  const std::string w(who);
  NIDT_REQUIRE(N > 0 && B > 0 && N % B == 0, w + ": N % B");
  NIDT_REQUIRE(C >= 8 && C % 8 == 0 && gp_pow2(C / 8) && C / 8 <= 64, w + ": C / 8 must be a power of two <= 64");
  NIDT_REQUIRE(groups > 0 && C % groups == 0 && (8 % (C / groups) == 0 || (C / groups) % 8 == 0),
               w + ": C / groups must divide 8 or be a multiple of 8");
  NIDT_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * C <= 65536, w + ": H W C <= 65536 (register-resident samples)");
  NIDT_REQUIRE(!pool || (H % 2 == 0 && W % 2 == 0), w + ": the pool needs even H and W");
  GpPlan g;
  g.B = B; g.H = H; g.W = W; g.C = C; g.groups = groups;
  g.lnch = gp_log2(C / 8);
  g.lcg = gp_log2(C / groups);
  g.U = (pool ? (H / 2) * (W / 2) : H * W) * (C / 8);
  g.ltps = std::min(9, gp_log2(g.U));
  g.tps = 1 << g.ltps;
  g.spb = kGpThreads / g.tps;
  g.bpc = ceil_div(B, g.spb);
  g.nred = (kGpThreads >> std::min(g.ltps, 6)) * C;
  g.nchs = g.spb * C;
  return g;
}

static int gp_nu(const GpPlan& g) {
  const int nu = ceil_div(g.U, kGpThreads);
  return nu <= 1 ? 1 : nu <= 2 ? 2 : nu <= 4 ? 4 : nu <= 8 ? 8 : 16;
}

// Typed dispatch over (units per thread, pool, relu): pooled samples hold 4 chunks per unit, so NU <= 4 there.
#define GP_SWITCH(LAUNCH)                                                                                      \
  if (pool) {                                                                                                  \
    switch (nu) {                                                                                              \
      case 1: if (relu) LAUNCH(1, true, true); else LAUNCH(1, true, false); break;                             \
      case 2: if (relu) LAUNCH(2, true, true); else LAUNCH(2, true, false); break;                             \
      default: if (relu) LAUNCH(4, true, true); else LAUNCH(4, true, false); break;                            \
    }                                                                                                          \
  } else {                                                                                                     \
    switch (nu) {                                                                                              \
      case 1: if (relu) LAUNCH(1, false, true); else LAUNCH(1, false, false); break;                           \
      case 2: if (relu) LAUNCH(2, false, true); else LAUNCH(2, false, false); break;                           \
      case 4: if (relu) LAUNCH(4, false, true); else LAUNCH(4, false, false); break;                           \
      case 8: if (relu) LAUNCH(8, false, true); else LAUNCH(8, false, false); break;                           \
      default: if (relu) LAUNCH(16, false, true); else LAUNCH(16, false, false); break;                        \
    }                                                                                                          \
  }

void gn2d_fwd(uintptr_t t, uintptr_t gamma, uintptr_t beta, int64_t ld, uintptr_t y, uintptr_t stats, int N, int B,
              int H, int W, int C, int groups, float eps, int relu, int pool, uintptr_t stream) {
  const GpPlan g = gp_plan(N, B, H, W, C, groups, pool, "gn2d_fwd");
  NIDT_REQUIRE(t % 16 == 0 && y % 16 == 0, "gn2d_fwd: 16-byte aligned activations");
  const int nu = gp_nu(g);
  const dim3 grid((unsigned)(N / B * g.bpc));
  const size_t lds = sizeof(float) * (g.nred + g.nchs);
  hipStream_t s = as_stream(stream);
#define GPF(NUV, P, R)                                                                                         \
  hipLaunchKernelGGL((k_gn2d_fwd<NUV, P, R>), grid, dim3(kGpThreads), lds, s, ptr<const uint16_t>(t),           \
                     ptr<const float>(gamma), ptr<const float>(beta), ld, ptr<uint16_t>(y), ptr<float>(stats), eps, g)
  GP_SWITCH(GPF)
#undef GPF
  NIDT_CHECK(hipGetLastError());
}

void gn2d_bwd(uintptr_t dy, uintptr_t t, uintptr_t stats, uintptr_t gamma, uintptr_t beta, int64_t ld, uintptr_t dt,
              uintptr_t part, int N, int B, int H, int W, int C, int groups, int relu, int pool, uintptr_t stream) {
  const GpPlan g = gp_plan(N, B, H, W, C, groups, pool, "gn2d_bwd");
  NIDT_REQUIRE(t % 16 == 0 && dy % 16 == 0 && dt % 16 == 0, "gn2d_bwd: 16-byte aligned activations");
  NIDT_REQUIRE(stats != 0 && part != 0, "gn2d_bwd: the saved statistics and the partials buffer");
  const int nu = gp_nu(g);
  const dim3 grid((unsigned)(N / B * g.bpc));
  const size_t lds = sizeof(float) * (g.nred + 2 * g.nchs + g.spb * g.groups);  // <= 64 KiB
  hipStream_t s = as_stream(stream);
#define GPB(NUV, P, R)                                                                                         \
  hipLaunchKernelGGL((k_gn2d_bwd<NUV, P, R>), grid, dim3(kGpThreads), lds, s, ptr<const uint16_t>(dy),          \
                     ptr<const uint16_t>(t), ptr<const float>(stats), ptr<const float>(gamma),                  \
                     ptr<const float>(beta), ld, ptr<uint16_t>(dt), ptr<float>(part), g)
  GP_SWITCH(GPB)
#undef GPB
  NIDT_CHECK(hipGetLastError());
}
#undef GP_SWITCH

// Plain 2x2 stride-2 max-pool on channels-last bf16 x [N][H][W][C] -> y [N][H/2][W/2][C]; the same unit (one chunk
// column x one window in one thread) and tie rule; the backward recomputes the argmax from the saved input.
template <bool BWD>
__global__ __launch_bounds__(256) void k_pool2d(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy,
                                                uint16_t* __restrict__ out, int64_t units, int H, int W, int C) {
  const int nch = C >> 3, Ho = H >> 1, Wo = W >> 1;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(u % nch);
    int64_t p = u / nch;
    const int wo = (int)(p % Wo);
    p /= Wo;
    const int ho = (int)(p % Ho);
    const int64_t n = p / Ho;
    const int64_t in0 = (((n * H + 2 * ho) * W + 2 * wo) * nch + j) * 8;  // elements; u * 8 is the pooled chunk
    float best[8], d[8];
    uint32_t sel = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float f[8];
      gp_unpack8(*reinterpret_cast<const i32x4_t*>(x + in0 + (int64_t)((i >> 1) * W + (i & 1)) * C), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (i == 0 || f[e] > best[e]) {
          best[e] = f[e];
          if (i) sel = (sel & ~(3u << (2 * e))) | ((uint32_t)i << (2 * e));
        }
      }
    }
    if (!BWD) {
      *reinterpret_cast<i32x4_t*>(out + u * 8) = gp_pack8(best);
    } else {
      gp_unpack8(*reinterpret_cast<const i32x4_t*>(dy + u * 8), d);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = ((sel >> (2 * e)) & 3u) == (uint32_t)i ? d[e] : 0.f;
        *reinterpret_cast<i32x4_t*>(out + in0 + (int64_t)((i >> 1) * W + (i & 1)) * C) = gp_pack8(r);
      }
    }
  }
}

static int64_t pool2d_units(int N, int H, int W, int C, const char* who) {
  NIDT_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && H % 2 == 0 && W % 2 == 0,
               std::string(who) + ": C % 8 == 0, even H and W");
  return (int64_t)N * (H / 2) * (W / 2) * (C / 8);
}

void pool2d_fwd(uintptr_t x, uintptr_t y, int N, int H, int W, int C, uintptr_t stream) {
  const int64_t units = pool2d_units(N, H, W, C, "pool2d_fwd");
  NIDT_REQUIRE(x % 16 == 0 && y % 16 == 0, "pool2d_fwd: 16-byte aligned activations");
  hipLaunchKernelGGL(k_pool2d<false>, dim3((unsigned)std::min<int64_t>(16384, (units + 255) / 256)), dim3(256), 0,
                     as_stream(stream), ptr<const uint16_t>(x), nullptr, ptr<uint16_t>(y), units, H, W, C);
  NIDT_CHECK(hipGetLastError());
}

void pool2d_bwd(uintptr_t dy, uintptr_t x, uintptr_t dx, int N, int H, int W, int C, uintptr_t stream) {
  const int64_t units = pool2d_units(N, H, W, C, "pool2d_bwd");
  NIDT_REQUIRE(x % 16 == 0 && dy % 16 == 0 && dx % 16 == 0, "pool2d_bwd: 16-byte aligned activations");
  hipLaunchKernelGGL(k_pool2d<true>, dim3((unsigned)std::min<int64_t>(16384, (units + 255) / 256)), dim3(256), 0,
                     as_stream(stream), ptr<const uint16_t>(x), ptr<const uint16_t>(dy), ptr<uint16_t>(dx), units, H,
                     W, C);
  NIDT_CHECK(hipGetLastError());
}

}  // namespace nidt
