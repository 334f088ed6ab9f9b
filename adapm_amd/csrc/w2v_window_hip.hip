// word2vec window step (contract: kernels.h, w2v_window_step_gpu).
//   k_ww_scan_block   exclusive int32 scan of one block of W2V_SCAN_BLOCK items
//                     in LDS, the items computed on the fly (keep flags, or
//                     per-centre pair counts); leaves the block's total
//   k_ww_scan_totals  one workgroup scans the block totals in place
//   k_ww_compact      one thread per position: ctok, sentence bounds, counts
//   k_w2v_window_step one wave per centre: the whole window of a centre
//   k_w2v_window_pairs one thread per centre: the same pairs, written out
//
// The step kernel holds the centre's emb and acc columns in registers for all
// of its up to 2W pairs: the row is read once and written once, where the pair
// kernel reads and writes it per pair. A wave, not a workgroup, owns a centre:
// D <= 512 is at most two float4 per lane, the dot needs no LDS and no barrier,
// and the four waves of a workgroup run independent centres. The target words
// of a pair are drawn by 1 + N lanes at once; the rows are then walked one
// after the other with the next row's two halves already requested.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace adapm {
namespace {

constexpr int WT = 256;  // threads per workgroup (4 waves)
constexpr int SCAN_ITEMS = W2V_SCAN_BLOCK / WT;
constexpr uint64_t GOLD = 0x9e3779b97f4a7c15ULL;

// pcg_hash64 of k_alias_draw
__device__ __host__ inline uint64_t ww_hash(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}
__device__ inline float ww_unit(uint64_t h) {
  return (float)((h >> 40) & 0xffffff) * (1.0f / 16777216.0f);
}

// adagrad_delta, sigmoidf and softplus1pf of kernels_hip.hip, repeated
// (kernels.h says why, above rescal_step_fused_gpu)
__device__ inline float ww_adagrad_delta(float g, float acc, float lr, float eps) {
  float G = acc + g * g;
  return -lr * g * __frsqrt_rn(G + eps);
}
__device__ inline float ww_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ inline float ww_softplus1p(float x) {
  if (x > 20.f) return x;
  float t = __expf(x);
  return t < 0.01f ? t * (1.f - t * (0.5f - t * (1.f / 3.f))) : __logf(1.f + t);
}

// Everything the plan and its readers share, passed by value.
struct Plan {
  const int32_t* tok;
  const int32_t* starts;
  const float* keep;
  const float* prob;
  const int32_t* alias;
  uint64_t n;
  int T, S, W, N;
  uint64_t sd0, sd1, sd2;
  int32_t* pos;   // [T + 1] keep-flag scan within its block
  int32_t* tot;   // [nb]    scanned block totals
  int32_t* ppos;  // [T + 1] pair-count scan (pairs entry)
  int32_t* ptot;  // [nb]
  int32_t* ctok;  // [T]
  int32_t* lo;    // [T]
  int32_t* hi;    // [T]
};

__device__ inline int scan_at(const int32_t* pos, const int32_t* tot, int64_t i) {
  return pos[i] + tot[i / W2V_SCAN_BLOCK];
}

// rule 1; item T of the scan is 0
__device__ inline int keep_flag(const Plan& p, int64_t i) {
  if (i >= p.T) return 0;
  if (!p.keep) return 1;
  uint64_t h = ww_hash(p.sd0 ^ (uint64_t)i * GOLD);
  return ww_unit(h) < p.keep[p.tok[i]] ? 1 : 0;
}

// rule 3
__device__ inline int window_b(const Plan& p, int64_t c) {
  return 1 + (int)(ww_hash(p.sd1 ^ (uint64_t)c * GOLD) % (uint64_t)p.W);
}

// rule 4, counted: j in [c - b, c + b] within [lo, hi), c itself left out
__device__ inline int pair_count(const Plan& p, int64_t c) {
  if (c >= scan_at(p.pos, p.tot, p.T)) return 0;
  const int64_t b = window_b(p, c);
  const int64_t lo = p.lo[c], hi = p.hi[c];
  const int64_t l = c - b > lo ? c - b : lo, r = c + b < hi - 1 ? c + b : hi - 1;
  return (int)(r - l);
}

// rule 5
__device__ inline int draw_word(const Plan& p, int64_t c, int a, int d) {
  const uint64_t idx = ((uint64_t)c * (uint64_t)(2 * p.W + 1) + (uint64_t)a) * (uint64_t)p.N + d;
  const uint64_t h = ww_hash(p.sd2 ^ idx * GOLD);
  const uint64_t slot = h % p.n;
  return ww_unit(h) < p.prob[slot] ? (int)slot : p.alias[slot];
}

// Inclusive scan of v over the workgroup; *total is the workgroup's sum. Ends
// with a barrier, so lds can be used again at once.
__device__ inline int block_scan_incl(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    int t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) lds[wv] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WT / 64; ++w) {
    int s = lds[w];
    if (w < wv) before += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return inc + before;
}

enum { ITEM_KEEP = 0, ITEM_PAIRS = 1 };

template <int ITEM>
__global__ __launch_bounds__(WT) void k_ww_scan_block(Plan p, int64_t n) {
  __shared__ int lds[WT / 64];
  int32_t* out = ITEM == ITEM_KEEP ? p.pos : p.ppos;
  int32_t* tot = ITEM == ITEM_KEEP ? p.tot : p.ptot;
  const int64_t base = (int64_t)blockIdx.x * W2V_SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
  int v[SCAN_ITEMS], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    const int64_t i = base + k;
    v[k] = i < n ? (ITEM == ITEM_KEEP ? keep_flag(p, i) : pair_count(p, i)) : 0;
    s += v[k];
  }
  int total;
  int ex = block_scan_incl(s, lds, &total) - s;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    if (base + k < n) out[base + k] = ex;
    ex += v[k];
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

__global__ __launch_bounds__(WT) void k_ww_scan_totals(int32_t* tot, int nb) {
  __shared__ int lds[WT / 64];
  int carry = 0;
  for (int base = 0; base < nb; base += WT) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? tot[i] : 0;
    int total;
    const int inc = block_scan_incl(v, lds, &total);
    if (i < nb) tot[i] = carry + inc - v;
    carry += total;
  }
}

// rule 2 and the bounds of rule 4; counts[1] is left at 0 for the step's waves
// to add to (the pairs entry overwrites it).
__global__ __launch_bounds__(WT) void k_ww_compact(Plan p, float* loss, int32_t* counts) {
  const int64_t i = (int64_t)blockIdx.x * WT + threadIdx.x;
  const int nk = scan_at(p.pos, p.tot, p.T);
  if (i == 0) {
    counts[0] = nk;
    counts[1] = 0;
  }
  if (i >= p.T) return;
  if (loss && i >= nk) loss[i] = 0.f;
  const int c = scan_at(p.pos, p.tot, i);
  if (scan_at(p.pos, p.tot, i + 1) == c) return;  // dropped
  // first s in [1, S] with starts[s] > i: starts[0] = 0 <= i < T = starts[S]
  int a = 1, b = p.S;
  while (a < b) {
    const int m = (a + b) >> 1;
    if (p.starts[m] > i) b = m;
    else a = m + 1;
  }
  p.ctok[c] = p.tok[i];
  p.lo[c] = scan_at(p.pos, p.tot, p.starts[a - 1]);
  p.hi[c] = scan_at(p.pos, p.tot, p.starts[a]);
}

// A row half in the registers of a wave: NF floats per lane.
template <int NV, bool VEC>
struct Cols {
  static constexpr int NF = VEC ? 4 * NV : NV;
  __device__ static inline int col(int lane, int e) {
    return VEC ? 4 * (lane + 64 * (e >> 2)) + (e & 3) : lane + 64 * e;
  }
  // columns at or past D read as `fill` and are never written
  __device__ static inline void load(float (&x)[NF], const float* row, int lane, int D,
                                     float fill) {
    if constexpr (VEC) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int k = 4 * (lane + 64 * v);
        float4 q = make_float4(fill, fill, fill, fill);
        if (k < D) q = *reinterpret_cast<const float4*>(row + k);
        x[4 * v] = q.x, x[4 * v + 1] = q.y, x[4 * v + 2] = q.z, x[4 * v + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        const int k = lane + 64 * e;
        x[e] = k < D ? row[k] : fill;
      }
    }
  }
};

template <int NV, bool VEC>
__global__ __launch_bounds__(WT) void k_w2v_window_step(Plan p, float* slab, int32_t plen, int D,
                                                        float lr, float eps, float* loss,
                                                        int32_t* counts) {
  using C = Cols<NV, VEC>;
  constexpr int NF = C::NF;
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (WT / 64) + (threadIdx.x >> 6);
  if (c >= counts[0]) return;  // n_kept, left by the plan
  const int lo = p.lo[c], hi = p.hi[c];
  const int b = window_b(p, c);
  float* cb = slab + 2 * (int64_t)p.ctok[c] * plen;

  float ce0[NF], ca0[NF], ce[NF], ca[NF], ac[NF];
  C::load(ce0, cb, lane, D, 0.f);
  C::load(ca0, cb + D, lane, D, 1.f);
#pragma unroll
  for (int e = 0; e < NF; ++e) ce[e] = ce0[e], ca[e] = ca0[e];

  float lsum = 0.f;
  int np = 0;
  for (int a = p.W - b; a <= p.W + b; ++a) {
    const int64_t j = c - p.W + a;
    if (a == p.W || j < lo || j >= hi) continue;
    ++np;
    // the pair's target words, one per lane
    int word = 0;
    if (lane == 0) word = p.ctok[j];
    else if (lane <= p.N) word = draw_word(p, c, a, lane - 1);

    float xe_n[NF], xa_n[NF];
    float* xb_n = slab + (2 * (int64_t)__shfl(word, 0, 64) + 1) * plen;
    C::load(xe_n, xb_n, lane, D, 0.f);
    C::load(xa_n, xb_n + D, lane, D, 1.f);
#pragma unroll
    for (int e = 0; e < NF; ++e) ac[e] = 0.f;

    for (int t = 0; t <= p.N; ++t) {
      float xe[NF], xa[NF];
      float* xb = xb_n;
#pragma unroll
      for (int e = 0; e < NF; ++e) xe[e] = xe_n[e], xa[e] = xa_n[e];
      if (t < p.N) {  // the next target's row, in flight over this one's work
        xb_n = slab + (2 * (int64_t)__shfl(word, t + 1, 64) + 1) * plen;
        C::load(xe_n, xb_n, lane, D, 0.f);
        C::load(xa_n, xb_n + D, lane, D, 1.f);
      }
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < NF; ++e) dot += ce[e] * xe[e];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
      const float z = t == 0 ? -dot : dot;  // -y * dot
      const float g = t == 0 ? -ww_sigmoid(z) : ww_sigmoid(z);
      lsum += ww_softplus1p(z);
#pragma unroll
      for (int e = 0; e < NF; ++e) {
        const int k = C::col(lane, e);
        if (k >= D) continue;
        ac[e] += g * xe[e];
        const float gx = g * ce[e];
        atomicAdd(&xb[k], ww_adagrad_delta(gx, xa[e], lr, eps));
        atomicAdd(&xb[D + k], gx * gx);
      }
    }
    // rule 8: the held centre moves after every pair
#pragma unroll
    for (int e = 0; e < NF; ++e) {
      if (C::col(lane, e) >= D) continue;
      const float g = ac[e];
      ce[e] += ww_adagrad_delta(g, ca[e], lr, eps);
      ca[e] += g * g;
    }
  }
  if (np) {
#pragma unroll
    for (int e = 0; e < NF; ++e) {
      const int k = C::col(lane, e);
      if (k >= D) continue;
      atomicAdd(&cb[k], ce[e] - ce0[e]);
      atomicAdd(&cb[D + k], ca[e] - ca0[e]);
    }
  }
  if (lane == 0) {
    loss[c] = lsum;
    if (np) atomicAdd(&counts[1], np);
  }
}

__global__ __launch_bounds__(WT) void k_w2v_window_pairs(Plan p, int64_t* ctr, int64_t* ctx,
                                                         int64_t* neg, int32_t* counts) {
  const int64_t c = (int64_t)blockIdx.x * WT + threadIdx.x;
  if (c == 0) counts[1] = scan_at(p.ppos, p.ptot, p.T);
  if (c >= scan_at(p.pos, p.tot, p.T)) return;
  const int lo = p.lo[c], hi = p.hi[c];
  const int b = window_b(p, c);
  int64_t q = scan_at(p.ppos, p.ptot, c);
  for (int a = p.W - b; a <= p.W + b; ++a) {
    const int64_t j = c - p.W + a;
    if (a == p.W || j < lo || j >= hi) continue;
    ctr[q] = p.ctok[c];
    ctx[q] = p.ctok[j];
    for (int d = 0; d < p.N; ++d) neg[q * p.N + d] = draw_word(p, c, a, d);
    ++q;
  }
}

__global__ void k_ww_zero_counts(int32_t* counts) { counts[0] = counts[1] = 0; }

// Carves `work` up and enqueues the plan launches. Returns false for T == 0,
// after setting counts.
bool enqueue_plan(const W2VWindowArgs& a, int32_t* work, float* loss, int32_t* counts,
                  hipStream_t st, Plan* out) {
  if (a.T < 1) {
    hipLaunchKernelGGL(k_ww_zero_counts, dim3(1), dim3(1), 0, st, counts);
    return false;
  }
  const int64_t n = a.T + 1, nb = (n + W2V_SCAN_BLOCK - 1) / W2V_SCAN_BLOCK;
  Plan p;
  p.tok = a.tok, p.starts = a.starts, p.keep = a.keep, p.prob = a.prob, p.alias = a.alias;
  p.n = (uint64_t)a.n, p.T = (int)a.T, p.S = (int)a.S, p.W = a.W, p.N = a.N;
  p.sd0 = ww_hash(a.seed), p.sd1 = ww_hash(a.seed + 1), p.sd2 = ww_hash(a.seed + 2);
  p.pos = work, p.tot = p.pos + n, p.ppos = p.tot + nb, p.ptot = p.ppos + n;
  p.ctok = p.ptot + nb, p.lo = p.ctok + a.T, p.hi = p.lo + a.T;
  hipLaunchKernelGGL(k_ww_scan_block<ITEM_KEEP>, dim3((unsigned)nb), dim3(WT), 0, st, p, n);
  hipLaunchKernelGGL(k_ww_scan_totals, dim3(1), dim3(WT), 0, st, p.tot, (int)nb);
  hipLaunchKernelGGL(k_ww_compact, dim3((unsigned)((a.T + WT - 1) / WT)), dim3(WT), 0, st, p,
                     loss, counts);
  *out = p;
  return true;
}

}  // namespace

void w2v_window_step_gpu(float* slab, int32_t plen, const W2VWindowArgs& a, int D, float lr,
                         float eps, int32_t* work, float* loss, int32_t* counts, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  Plan p;
  if (!enqueue_plan(a, work, loss, counts, st, &p)) return;
  const dim3 grid((unsigned)((a.T + WT / 64 - 1) / (WT / 64)));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(WT), 0, st, p, slab, plen, D, lr, eps, loss, counts);
  };
  if (D % 4 == 0) {
    if (D <= 256) launch(k_w2v_window_step<1, true>);
    else launch(k_w2v_window_step<2, true>);
  } else if (D <= 64) launch(k_w2v_window_step<1, false>);
  else if (D <= 128) launch(k_w2v_window_step<2, false>);
  else if (D <= 256) launch(k_w2v_window_step<4, false>);
  else launch(k_w2v_window_step<8, false>);
}

void w2v_window_pairs_gpu(const W2VWindowArgs& a, int32_t* work, int64_t* ctr, int64_t* ctx,
                          int64_t* neg, int32_t* counts, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  Plan p;
  if (!enqueue_plan(a, work, nullptr, counts, st, &p)) return;
  const int64_t n = a.T + 1, nb = (n + W2V_SCAN_BLOCK - 1) / W2V_SCAN_BLOCK;
  hipLaunchKernelGGL(k_ww_scan_block<ITEM_PAIRS>, dim3((unsigned)nb), dim3(WT), 0, st, p, n);
  hipLaunchKernelGGL(k_ww_scan_totals, dim3(1), dim3(WT), 0, st, p.ptot, (int)nb);
  hipLaunchKernelGGL(k_w2v_window_pairs, dim3((unsigned)((a.T + WT - 1) / WT)), dim3(WT), 0, st, p,
                     ctr, ctx, neg, counts);
}

}  // namespace adapm
