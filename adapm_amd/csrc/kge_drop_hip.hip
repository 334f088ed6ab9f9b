// ComplEx sides step with dropout (contract: kernels.h, kge_complex_step_drop_gpu).
//   k_kge_step_drop        pulled rows in, push deltas out
//   k_kge_step_drop_fused  the slab's own rows, AdaGrad in place
//
// One workgroup of 256 threads per positive, grid-stride over B; a thread owns
// the complex lanes k = tid + i * 256, i < KPT, in registers. The sides kernels
// of kernels_hip.hip hoist u = s*r out of the object pass and v = conj(r)*o out
// of the subject pass. Here every scored triple t masks its three rows afresh,
// so neither product is loop-invariant, and the register plan is:
//   object pass   raw s, r (4), the accumulators a_s, a_r, a_o (6) per lane;
//                 a_o sits where the sides kernels keep u. Per triple: o_t (2,
//                 the fused kernel also its accumulator halves), one 64-bit
//                 hash per lane (2), and s~, r~, o~, u~ = s~ r~ as temporaries
//                 on either side of the block reduction.
//   subject pass  raw r, the positive o read again (4), a_r, a_o (4); per
//                 triple s'_j (2), the hash (2), v~ = conj(r~) o~ temporary.
// The hash is kept across the reduction of psi and the six mask factors are
// taken from it again afterwards (three and-compare-selects per half): the
// masked rows need no registers over the barrier, and no mask is ever stored.
// The factors of a dropped component are 0, so its gradient is an exact zero.
//
// adagrad_delta, the softplus, the block reduction and the slab write of
// kernels_hip.hip are repeated here rather than shared (kernels.h, above
// rescal_step_fused_gpu, says why).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.h"

namespace adapm {
namespace {

constexpr int KT = 256;  // threads per workgroup
static_assert(STEP_MAX_LANES == 8 * KT, "dispatch stops at KPT = 8");

struct Drop {
  uint64_t seed;
  uint32_t thr_e, thr_r;  // a component is kept iff its 10-bit field >= thr
  float sc_e, sc_r;       // 1024 / (1024 - thr)
};

// pcg_hash64 of k_alias_draw, on the counter idx
__device__ inline uint64_t kd_hash(uint64_t seed, uint64_t idx) {
  uint64_t x = seed ^ idx * 0x9e3779b97f4a7c15ULL;
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// The six factors (0 or scale) of one complex lane: field f is bits
// [10f, 10f + 10) of h, f = s_re, s_im, r_re, r_im, o_re, o_im.
struct Mask6 {
  float s_re, s_im, r_re, r_im, o_re, o_im;
};
__device__ inline Mask6 kd_masks(uint64_t h, const Drop& dp) {
  const uint32_t lo = (uint32_t)h;          // fields 0, 1, 2 and the low 2 bits of 3
  const uint32_t hi = (uint32_t)(h >> 30);  // fields 3, 4, 5
  Mask6 m;
  m.s_re = (lo & 1023u) >= dp.thr_e ? dp.sc_e : 0.f;
  m.s_im = ((lo >> 10) & 1023u) >= dp.thr_e ? dp.sc_e : 0.f;
  m.r_re = ((lo >> 20) & 1023u) >= dp.thr_r ? dp.sc_r : 0.f;
  m.r_im = (hi & 1023u) >= dp.thr_r ? dp.sc_r : 0.f;
  m.o_re = ((hi >> 10) & 1023u) >= dp.thr_e ? dp.sc_e : 0.f;
  m.o_im = ((hi >> 20) & 1023u) >= dp.thr_e ? dp.sc_e : 0.f;
  return m;
}

__device__ inline float kd_block_sum(float v, float* lds) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float out = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();
  return out;
}

__device__ inline float kd_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }

// softplus1pf of kernels_hip.hip
__device__ inline float kd_softplus1pf(float x) {
  if (x > 20.f) return x;
  float t = __expf(x);
  return t < 0.01f ? t * (1.f - t * (0.5f - t * (1.f / 3.f))) : __logf(1.f + t);
}

__device__ inline float kd_adagrad_delta(float g, float acc, float lr, float eps) {
  float G = acc + g * g;
  return -lr * g * __frsqrt_rn(G + eps);
}

// classic kernel: the push-ready pair [delta | g^2] of one complex lane
__device__ inline void kd_write_delta(float* d, int k, int dc, int D, float g_re, float g_im,
                                      float acc_re, float acc_im, float lr, float eps) {
  d[k] = kd_adagrad_delta(g_re, acc_re, lr, eps);
  d[dc + k] = kd_adagrad_delta(g_im, acc_im, lr, eps);
  d[D + k] = g_re * g_re;
  d[D + dc + k] = g_im * g_im;
}

__device__ inline float kd_plain_add(float a, float delta) {
#pragma clang fp contract(off)
  return a + delta;
}

// fused kernel: slab_adagrad of kernels_hip.hip for one complex lane. A row
// shared with another occurrence of the batch takes atomics; the only writer
// of a row stores over the values it read.
__device__ inline void kd_slab_adagrad(float* row, int k, int dc, int D, float g_re, float g_im,
                                       float emb_re, float emb_im, float acc_re, float acc_im,
                                       float lr, float eps, bool shared) {
  const float d_re = kd_adagrad_delta(g_re, acc_re, lr, eps);
  const float d_im = kd_adagrad_delta(g_im, acc_im, lr, eps);
  if (shared) {
    atomicAdd(&row[k], d_re);
    atomicAdd(&row[dc + k], d_im);
    atomicAdd(&row[D + k], g_re * g_re);
    atomicAdd(&row[D + dc + k], g_im * g_im);
  } else {
    row[k] = kd_plain_add(emb_re, d_re);
    row[dc + k] = kd_plain_add(emb_im, d_im);
    row[D + k] = kd_plain_add(acc_re, g_re * g_re);
    row[D + dc + k] = kd_plain_add(acc_im, g_im * g_im);
  }
}

// row_at and row_shared of kernels_hip.hip
__device__ inline float* kd_row_at(float* slab, int64_t v, int32_t plen, int world) {
  return world ? slab + (v / world) * (int64_t)plen : slab + v;
}
template <bool UNIQ>
__device__ inline bool kd_row_shared(const uint32_t* __restrict__ bits, int64_t key) {
  if (!UNIQ) return true;
  return (bits[key >> 5] >> (int)(key & 31)) & 1u;
}

// One masked complex lane of a scored triple (x, r, y) = (subject, relation,
// object), whichever of the three the pass holds fixed: the masked values and
// what both passes need of them.
struct Lane {
  float x_re, x_im, r_re, r_im, y_re, y_im;  // masked
  __device__ Lane(const Mask6& m, float xr, float xi, float rr, float ri, float yr, float yi)
      : x_re(m.s_re * xr), x_im(m.s_im * xi), r_re(m.r_re * rr), r_im(m.r_im * ri),
        y_re(m.o_re * yr), y_im(m.o_im * yi) {}
  // u~ = x~ r~, the direction of the object's gradient
  __device__ float u_re() const { return x_re * r_re - x_im * r_im; }
  __device__ float u_im() const { return x_im * r_re + x_re * r_im; }
  // v~ = conj(r~) y~, the direction of the subject's gradient
  __device__ float v_re() const { return r_re * y_re + r_im * y_im; }
  __device__ float v_im() const { return r_re * y_im - r_im * y_re; }
  // d psi / d r~
  __device__ float w_re() const { return x_re * y_re + x_im * y_im; }
  __device__ float w_im() const { return x_re * y_im - x_im * y_re; }
};

template <int KPT>
__global__ void __launch_bounds__(KT)
k_kge_step_drop(const float* __restrict__ s, const float* __restrict__ r,
                const float* __restrict__ o, const float* __restrict__ neg_o,
                const float* __restrict__ neg_s, float* __restrict__ ds, float* __restrict__ dr,
                float* __restrict__ do_, float* __restrict__ dneg_o, float* __restrict__ dneg_s,
                float* __restrict__ loss, int B, int N, int NS, int D, float lr, float eps,
                float gamma_e, float gamma_r, Drop dp) {
  __shared__ float lds[KT / 64];
  const int dc = D >> 1;
  const int row = D << 1;  // floats per pulled row
  const uint64_t T = 1 + (uint64_t)N + (uint64_t)NS;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* sb = s + (int64_t)b * row;
    const float* rb = r + (int64_t)b * row;
    const float* pb = o + (int64_t)b * row;
    const uint64_t idx0 = (uint64_t)b * T * (uint64_t)dc;  // counter of (t = 0, k = 0)

    float r_re[KPT], r_im[KPT], a_rre[KPT], a_rim[KPT], a_ore[KPT], a_oim[KPT];
    float lsum = 0.f;
    {
      float s_re[KPT], s_im[KPT], a_sre[KPT], a_sim[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + i * KT;
        a_sre[i] = a_sim[i] = a_rre[i] = a_rim[i] = a_ore[i] = a_oim[i] = 0.f;
        s_re[i] = k < dc ? sb[k] : 0.f;
        s_im[i] = k < dc ? sb[dc + k] : 0.f;
        r_re[i] = k < dc ? rb[k] : 0.f;
        r_im[i] = k < dc ? rb[dc + k] : 0.f;
      }

      // object pass: t = 0 the positive, t = j the triple (s, r, o'_j)
      for (int j = 0; j <= N; ++j) {
        const bool pos = j == 0;
        const float* ob = pos ? pb : neg_o + ((int64_t)b * N + (j - 1)) * row;
        const uint64_t base = idx0 + (uint64_t)j * (uint64_t)dc;
        float o_re[KPT], o_im[KPT];
        uint64_t h[KPT];
        float part = 0.f;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
          const int k = threadIdx.x + i * KT;
          o_re[i] = k < dc ? ob[k] : 0.f;
          o_im[i] = k < dc ? ob[dc + k] : 0.f;
          h[i] = kd_hash(dp.seed, base + (uint64_t)k);
          const Lane l(kd_masks(h[i], dp), s_re[i], s_im[i], r_re[i], r_im[i], o_re[i], o_im[i]);
          part += l.u_re() * l.y_re + l.u_im() * l.y_im;
        }
        const float psi = kd_block_sum(part, lds);
        const float y = pos ? 1.f : -1.f;
        const float c = -y * kd_sigmoid(-y * psi);  // dL/dpsi, L = softplus(-y*psi)
        if (threadIdx.x == 0) lsum += kd_softplus1pf(-y * psi);

        float* dob = pos ? nullptr : dneg_o + ((int64_t)b * N + (j - 1)) * row;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
          const int k = threadIdx.x + i * KT;
          if (k >= dc) continue;
          const Mask6 m = kd_masks(h[i], dp);
          const Lane l(m, s_re[i], s_im[i], r_re[i], r_im[i], o_re[i], o_im[i]);
          a_sre[i] += c * m.s_re * l.v_re();
          a_sim[i] += c * m.s_im * l.v_im();
          a_rre[i] += c * m.r_re * l.w_re();
          a_rim[i] += c * m.r_im * l.w_im();
          const float g_re = c * m.o_re * l.u_re();
          const float g_im = c * m.o_im * l.u_im();
          if (pos) {  // the positive object waits for the subject pass
            a_ore[i] = g_re;
            a_oim[i] = g_im;
            continue;
          }
          kd_write_delta(dob, k, dc, D, g_re, g_im, ob[D + k], ob[D + dc + k], lr, eps);
        }
      }

      float* dsb = ds + (int64_t)b * row;
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        kd_write_delta(dsb, k, dc, D, a_sre[i] + gamma_e * s_re[i], a_sim[i] + gamma_e * s_im[i],
                       sb[D + k], sb[D + dc + k], lr, eps);
      }
    }

    // subject pass: t = N + 1 + j the triple (s'_j, r, o)
    float p_re[KPT], p_im[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int k = threadIdx.x + i * KT;
      p_re[i] = k < dc ? pb[k] : 0.f;
      p_im[i] = k < dc ? pb[dc + k] : 0.f;
    }
    for (int j = 0; j < NS; ++j) {
      const float* xb = neg_s + ((int64_t)b * NS + j) * row;
      float* dxb = dneg_s + ((int64_t)b * NS + j) * row;
      const uint64_t base = idx0 + (uint64_t)(N + 1 + j) * (uint64_t)dc;
      float x_re[KPT], x_im[KPT];
      uint64_t h[KPT];
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + i * KT;
        x_re[i] = k < dc ? xb[k] : 0.f;
        x_im[i] = k < dc ? xb[dc + k] : 0.f;
        h[i] = kd_hash(dp.seed, base + (uint64_t)k);
        const Lane l(kd_masks(h[i], dp), x_re[i], x_im[i], r_re[i], r_im[i], p_re[i], p_im[i]);
        part += l.v_re() * l.x_re + l.v_im() * l.x_im;
      }
      const float psi = kd_block_sum(part, lds);
      const float c = kd_sigmoid(psi);  // dL/dpsi, L = softplus(psi)
      if (threadIdx.x == 0) lsum += kd_softplus1pf(psi);
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        const Mask6 m = kd_masks(h[i], dp);
        const Lane l(m, x_re[i], x_im[i], r_re[i], r_im[i], p_re[i], p_im[i]);
        a_rre[i] += c * m.r_re * l.w_re();
        a_rim[i] += c * m.r_im * l.w_im();
        a_ore[i] += c * m.o_re * l.u_re();
        a_oim[i] += c * m.o_im * l.u_im();
        kd_write_delta(dxb, k, dc, D, c * m.s_re * l.v_re(), c * m.s_im * l.v_im(), xb[D + k],
                       xb[D + dc + k], lr, eps);
      }
    }

    float* drb = dr + (int64_t)b * row;
    float* dpb = do_ + (int64_t)b * row;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int k = threadIdx.x + i * KT;
      if (k >= dc) continue;
      kd_write_delta(drb, k, dc, D, a_rre[i] + gamma_r * r_re[i], a_rim[i] + gamma_r * r_im[i],
                     rb[D + k], rb[D + dc + k], lr, eps);
      kd_write_delta(dpb, k, dc, D, a_ore[i] + gamma_e * p_re[i], a_oim[i] + gamma_e * p_im[i],
                     pb[D + k], pb[D + dc + k], lr, eps);
    }
    if (threadIdx.x == 0) loss[b] = lsum;
  }
}

// The same step on the slab's own rows, with the addressing and the UNIQ /
// bits contract of k_kge_step_sides_fused. Every row is written once per
// occurrence: o'_j and s'_j inside their pass, s between the passes, r and the
// positive o at the end.
template <int KPT, bool UNIQ>
__global__ void __launch_bounds__(KT)
k_kge_step_drop_fused(float* __restrict__ slab, const int64_t* __restrict__ keys_s,
                      const int64_t* __restrict__ keys_r, const int64_t* __restrict__ keys_o,
                      const int64_t* __restrict__ keys_neg_o,
                      const int64_t* __restrict__ keys_neg_s, float* __restrict__ loss, int B,
                      int N, int NS, int D, int32_t plen, int world, float lr, float eps,
                      float gamma_e, float gamma_r, Drop dp, const uint32_t* __restrict__ bits,
                      unsigned long long* __restrict__ shared_stat) {
  __shared__ float lds[KT / 64];
  const int dc = D >> 1;
  // the bits imply the single-rank layout: a constant spares kd_row_at the
  // 64-bit division
  const int w = UNIQ ? 1 : world;
  const uint64_t T = 1 + (uint64_t)N + (uint64_t)NS;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t key_s = keys_s[b], key_r = keys_r[b], key_o = keys_o[b];
    float* sb = kd_row_at(slab, key_s, plen, w);
    float* rb = kd_row_at(slab, key_r, plen, w);
    float* pb = kd_row_at(slab, key_o, plen, w);
    const bool s_shared = kd_row_shared<UNIQ>(bits, key_s);
    const bool r_shared = kd_row_shared<UNIQ>(bits, key_r);
    const bool p_shared = kd_row_shared<UNIQ>(bits, key_o);
    unsigned n_shared = (unsigned)s_shared + (unsigned)r_shared + (unsigned)p_shared;
    const uint64_t idx0 = (uint64_t)b * T * (uint64_t)dc;

    float r_re[KPT], r_im[KPT], a_rre[KPT], a_rim[KPT], a_ore[KPT], a_oim[KPT];
    float lsum = 0.f;
    {
      float s_re[KPT], s_im[KPT], a_sre[KPT], a_sim[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + i * KT;
        a_sre[i] = a_sim[i] = a_rre[i] = a_rim[i] = a_ore[i] = a_oim[i] = 0.f;
        s_re[i] = k < dc ? sb[k] : 0.f;
        s_im[i] = k < dc ? sb[dc + k] : 0.f;
        r_re[i] = k < dc ? rb[k] : 0.f;
        r_im[i] = k < dc ? rb[dc + k] : 0.f;
      }

      for (int j = 0; j <= N; ++j) {
        const bool pos = j == 0;
        const int64_t ok = pos ? key_o : keys_neg_o[(int64_t)b * N + (j - 1)];
        float* ob = kd_row_at(slab, ok, plen, w);
        const bool o_shared = pos ? p_shared : kd_row_shared<UNIQ>(bits, ok);
        if (!pos) n_shared += (unsigned)o_shared;
        const uint64_t base = idx0 + (uint64_t)j * (uint64_t)dc;
        float o_re[KPT], o_im[KPT], Go_re[KPT], Go_im[KPT];
        uint64_t h[KPT];
        float part = 0.f;
        // the accumulator halves ride with the embedding halves, so their
        // latency hides behind the hash and the block reduction
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
          const int k = threadIdx.x + i * KT;
          o_re[i] = k < dc ? ob[k] : 0.f;
          o_im[i] = k < dc ? ob[dc + k] : 0.f;
          Go_re[i] = (k < dc && !pos) ? ob[D + k] : 0.f;
          Go_im[i] = (k < dc && !pos) ? ob[D + dc + k] : 0.f;
          h[i] = kd_hash(dp.seed, base + (uint64_t)k);
          const Lane l(kd_masks(h[i], dp), s_re[i], s_im[i], r_re[i], r_im[i], o_re[i], o_im[i]);
          part += l.u_re() * l.y_re + l.u_im() * l.y_im;
        }
        const float psi = kd_block_sum(part, lds);
        const float y = pos ? 1.f : -1.f;
        const float c = -y * kd_sigmoid(-y * psi);
        if (threadIdx.x == 0) lsum += kd_softplus1pf(-y * psi);

#pragma unroll
        for (int i = 0; i < KPT; ++i) {
          const int k = threadIdx.x + i * KT;
          if (k >= dc) continue;
          const Mask6 m = kd_masks(h[i], dp);
          const Lane l(m, s_re[i], s_im[i], r_re[i], r_im[i], o_re[i], o_im[i]);
          a_sre[i] += c * m.s_re * l.v_re();
          a_sim[i] += c * m.s_im * l.v_im();
          a_rre[i] += c * m.r_re * l.w_re();
          a_rim[i] += c * m.r_im * l.w_im();
          const float g_re = c * m.o_re * l.u_re();
          const float g_im = c * m.o_im * l.u_im();
          if (pos) {  // the positive object waits for the subject pass
            a_ore[i] = g_re;
            a_oim[i] = g_im;
            continue;
          }
          kd_slab_adagrad(ob, k, dc, D, g_re, g_im, o_re[i], o_im[i], Go_re[i], Go_im[i], lr, eps,
                          o_shared);
        }
      }

#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        kd_slab_adagrad(sb, k, dc, D, a_sre[i] + gamma_e * s_re[i], a_sim[i] + gamma_e * s_im[i],
                        s_re[i], s_im[i], sb[D + k], sb[D + dc + k], lr, eps, s_shared);
      }
    }

    float p_re[KPT], p_im[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int k = threadIdx.x + i * KT;
      p_re[i] = k < dc ? pb[k] : 0.f;
      p_im[i] = k < dc ? pb[dc + k] : 0.f;
    }
    for (int j = 0; j < NS; ++j) {
      const int64_t xk = keys_neg_s[(int64_t)b * NS + j];
      float* xb = kd_row_at(slab, xk, plen, w);
      const bool x_shared = kd_row_shared<UNIQ>(bits, xk);
      n_shared += (unsigned)x_shared;
      const uint64_t base = idx0 + (uint64_t)(N + 1 + j) * (uint64_t)dc;
      float x_re[KPT], x_im[KPT], Gx_re[KPT], Gx_im[KPT];
      uint64_t h[KPT];
      float part = 0.f;
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + i * KT;
        x_re[i] = k < dc ? xb[k] : 0.f;
        x_im[i] = k < dc ? xb[dc + k] : 0.f;
        Gx_re[i] = k < dc ? xb[D + k] : 0.f;
        Gx_im[i] = k < dc ? xb[D + dc + k] : 0.f;
        h[i] = kd_hash(dp.seed, base + (uint64_t)k);
        const Lane l(kd_masks(h[i], dp), x_re[i], x_im[i], r_re[i], r_im[i], p_re[i], p_im[i]);
        part += l.v_re() * l.x_re + l.v_im() * l.x_im;
      }
      const float psi = kd_block_sum(part, lds);
      const float c = kd_sigmoid(psi);
      if (threadIdx.x == 0) lsum += kd_softplus1pf(psi);
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        const Mask6 m = kd_masks(h[i], dp);
        const Lane l(m, x_re[i], x_im[i], r_re[i], r_im[i], p_re[i], p_im[i]);
        a_rre[i] += c * m.r_re * l.w_re();
        a_rim[i] += c * m.r_im * l.w_im();
        a_ore[i] += c * m.o_re * l.u_re();
        a_oim[i] += c * m.o_im * l.u_im();
        kd_slab_adagrad(xb, k, dc, D, c * m.s_re * l.v_re(), c * m.s_im * l.v_im(), x_re[i],
                        x_im[i], Gx_re[i], Gx_im[i], lr, eps, x_shared);
      }
    }

#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int k = threadIdx.x + i * KT;
      if (k >= dc) continue;
      kd_slab_adagrad(rb, k, dc, D, a_rre[i] + gamma_r * r_re[i], a_rim[i] + gamma_r * r_im[i],
                      r_re[i], r_im[i], rb[D + k], rb[D + dc + k], lr, eps, r_shared);
      kd_slab_adagrad(pb, k, dc, D, a_ore[i] + gamma_e * p_re[i], a_oim[i] + gamma_e * p_im[i],
                      p_re[i], p_im[i], pb[D + k], pb[D + dc + k], lr, eps, p_shared);
    }
    if (threadIdx.x == 0) {
      loss[b] = lsum;
      if (UNIQ && shared_stat) atomicAdd(shared_stat, (unsigned long long)n_shared);
    }
  }
}

// f(std::integral_constant<int, KPT>) for the smallest KPT of 1, 2, 4, 8 that
// covers `lanes`; the entry points have refused more than STEP_MAX_LANES.
template <typename F>
inline void dispatch_kpt(int lanes, F&& f) {
  if (lanes <= KT) f(std::integral_constant<int, 1>{});
  else if (lanes <= 2 * KT) f(std::integral_constant<int, 2>{});
  else if (lanes <= 4 * KT) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>(n, 16384); }

inline Drop drop_args(int thr_e, int thr_r, uint64_t seed) {
  return Drop{seed, (uint32_t)thr_e, (uint32_t)thr_r, drop_scale(thr_e), drop_scale(thr_r)};
}

}  // namespace

void kge_complex_step_drop_gpu(const float* s, const float* r, const float* o,
                               const float* neg_o, const float* neg_s, float* ds, float* dr,
                               float* do_, float* dneg_o, float* dneg_s, float* loss, int B,
                               int N, int NS, int D, float lr, float eps, float gamma_e,
                               float gamma_r, int thr_e, int thr_r, uint64_t drop_seed,
                               void* stream) {
  if (B < 1) return;
  // no dropout is the sides step, and is run by its kernels: only the same
  // code gives the same bits (kge_complex_step_sides_gpu says more)
  if (thr_e == 0 && thr_r == 0)
    return kge_complex_step_sides_gpu(s, r, o, neg_o, neg_s, ds, dr, do_, dneg_o, dneg_s, loss, B,
                                      N, NS, D, lr, eps, gamma_e, gamma_r, stream);
  const Drop dp = drop_args(thr_e, thr_r, drop_seed);
  dispatch_kpt(D >> 1, [&](auto kpt) {
    hipLaunchKernelGGL(k_kge_step_drop<decltype(kpt)::value>, dim3(grid_for(B)), dim3(KT), 0,
                       (hipStream_t)stream, s, r, o, neg_o, neg_s, ds, dr, do_, dneg_o, dneg_s,
                       loss, B, N, NS, D, lr, eps, gamma_e, gamma_r, dp);
  });
}

void kge_complex_step_drop_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                     const int64_t* keys_o, const int64_t* keys_neg_o,
                                     const int64_t* keys_neg_s, float* loss, int B, int N, int NS,
                                     int D, int32_t plen, int world, float lr, float eps,
                                     float gamma_e, float gamma_r, int thr_e, int thr_r,
                                     uint64_t drop_seed, void* stream, const uint32_t* bits,
                                     unsigned long long* shared_stat) {
  if (B < 1) return;
  if (thr_e == 0 && thr_r == 0)
    return kge_complex_step_sides_fused_gpu(slab, keys_s, keys_r, keys_o, keys_neg_o, keys_neg_s,
                                            loss, B, N, NS, D, plen, world, lr, eps, gamma_e,
                                            gamma_r, stream, bits, shared_stat);
  const bool uniq = bits != nullptr && world == 1;  // as in kge_complex_step_fused_gpu
  if (!uniq) bits = nullptr, shared_stat = nullptr;
  const Drop dp = drop_args(thr_e, thr_r, drop_seed);
  dispatch_kpt(D >> 1, [&](auto kpt) {
    constexpr int KPT = decltype(kpt)::value;
    hipLaunchKernelGGL(
        (uniq ? k_kge_step_drop_fused<KPT, true> : k_kge_step_drop_fused<KPT, false>),
        dim3(grid_for(B)), dim3(KT), 0, (hipStream_t)stream, slab, keys_s, keys_r, keys_o,
        keys_neg_o, keys_neg_s, loss, B, N, NS, D, plen, world, lr, eps, gamma_e, gamma_r, dp, bits,
        shared_stat);
  });
}

}  // namespace adapm
