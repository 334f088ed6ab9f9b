// HIP/gfx950 app kernels — see kernels.h. One workgroup (256 threads =
// 4 waves) per training sample; rows are 2D floats = [emb(D) | accum(D)].
// These kernels are HBM-bound (each pulled row is read once, each delta
// row written once); the arithmetic per element is small, so the design
// goal is coalesced row traffic (one dword per lane, 256 contiguous bytes
// per wave instruction) and cheap block reductions (wave __shfl_xor + one
// LDS hop across the 4 waves).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>

#include "kernels.h"
#include "ustream.h"

namespace adapm {

#define KT 256  // threads per workgroup

// Blocks for n grid-strided work items: at least one (an empty batch is a
// launch whose loop never runs), at most `cap`.
static inline unsigned grid_for(int64_t n, int64_t cap = 16384) {
  return (unsigned)std::min(std::max<int64_t>(n, 1), cap);
}

// The step kernels keep a row's lanes in registers, KPT per thread, so KPT
// is a template argument: f receives it as std::integral_constant<int, KPT>
// for the smallest KPT of 1, 2, 4, 8 that covers `lanes`. The entry points
// refuse rows of more than STEP_MAX_LANES lanes before they get here.
static_assert(STEP_MAX_LANES == 8 * KT, "dispatch_kpt stops at KPT = 8");
template <typename F>
static inline void dispatch_kpt(int lanes, F&& f) {
  if (lanes <= KT) f(std::integral_constant<int, 1>{});
  else if (lanes <= 2 * KT) f(std::integral_constant<int, 2>{});
  else if (lanes <= 4 * KT) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

__device__ inline float block_reduce_sum(float v, float* lds) {
  // wave-level reduce (64 lanes)
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  int wave = threadIdx.x >> 6;
  int lane = threadIdx.x & 63;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  float r = (threadIdx.x < KT / 64) ? lds[threadIdx.x] : 0.f;
  if (threadIdx.x < 64) {
    for (int off = 2; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
  }
  if (threadIdx.x == 0) lds[0] = r;
  __syncthreads();
  float out = lds[0];
  __syncthreads();
  return out;
}

__device__ inline float sigmoidf(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ inline float softplusf(float x) {
  // log(1+exp(x)), stable
  return x > 20.f ? x : __logf(1.f + __expf(x));
}

// AdaGrad: the embedding delta for gradient g, given the accumulator value
// `acc` the lane read (G in the row's second half).
__device__ inline float adagrad_delta(float g, float acc, float lr, float eps) {
  float G = acc + g * g;
  return -lr * g * __frsqrt_rn(G + eps);
}

// Classic kernels: the push-ready pair [delta | g^2] of one lane.
__device__ inline void write_delta(float* d_emb, float* d_acc, float g, float acc, float lr,
                                   float eps) {
  *d_emb = adagrad_delta(g, acc, lr, eps);
  *d_acc = g * g;
}

// --------------------------------------------------------------- ComplEx

// Per workgroup: one positive triple + its N negatives (o-side corruption).
// Each thread owns complex positions k = tid + i*KT, i < KPT (compile-time
// KPT so the per-thread arrays stay in registers — runtime-indexed arrays
// spill to scratch on gfx950). D = 512 -> dc = 256 -> KPT = 1.
template <int KPT>
__global__ void k_kge_step(const float* __restrict__ s, const float* __restrict__ r,
                           const float* __restrict__ o, const float* __restrict__ neg,
                           float* __restrict__ ds, float* __restrict__ dr,
                           float* __restrict__ do_, float* __restrict__ dneg,
                           float* __restrict__ loss, int B, int N, int D, float lr, float eps) {
  __shared__ float lds[KT / 64];
  const int dc = D >> 1;
  const int row = D << 1;  // floats per pulled row
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* sb = s + (int64_t)b * row;
    const float* rb = r + (int64_t)b * row;

    float s_re[KPT], s_im[KPT], r_re[KPT], r_im[KPT];
    float a_sre[KPT], a_sim[KPT], a_rre[KPT], a_rim[KPT];
    float u_re[KPT], u_im[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      a_sre[i] = a_sim[i] = a_rre[i] = a_rim[i] = 0.f;
      if (k < dc) {
        s_re[i] = sb[k];
        s_im[i] = sb[dc + k];
        r_re[i] = rb[k];
        r_im[i] = rb[dc + k];
        // per-object o-gradient direction (independent of o)
        u_re[i] = s_re[i] * r_re[i] - s_im[i] * r_im[i];
        u_im[i] = s_im[i] * r_re[i] + s_re[i] * r_im[i];
      } else {
        s_re[i] = s_im[i] = r_re[i] = r_im[i] = u_re[i] = u_im[i] = 0.f;
      }
    }

    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      const float* ob = (j == 0) ? o + (int64_t)b * row
                                 : neg + ((int64_t)b * N + (j - 1)) * row;
      float y = (j == 0) ? 1.f : -1.f;
      float part = 0.f;
      float o_re[KPT], o_im[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        o_re[i] = k < dc ? ob[k] : 0.f;
        o_im[i] = k < dc ? ob[dc + k] : 0.f;
        part += u_re[i] * o_re[i] + u_im[i] * o_im[i];
      }
      float psi = block_reduce_sum(part, lds);
      float c = -y * sigmoidf(-y * psi);  // dL/dpsi, L = softplus(-y*psi)
      if (threadIdx.x == 0) lsum += softplusf(-y * psi);

      float* dob = (j == 0) ? do_ + (int64_t)b * row
                            : dneg + ((int64_t)b * N + (j - 1)) * row;
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        // accumulate s/r grads
        a_sre[i] += c * (r_re[i] * o_re[i] + r_im[i] * o_im[i]);
        a_sim[i] += c * (r_re[i] * o_im[i] - r_im[i] * o_re[i]);
        a_rre[i] += c * (s_re[i] * o_re[i] + s_im[i] * o_im[i]);
        a_rim[i] += c * (s_re[i] * o_im[i] - s_im[i] * o_re[i]);
        // o grad + fused AdaGrad (G in the row's second half)
        write_delta(&dob[k], &dob[D + k], c * u_re[i], ob[D + k], lr, eps);
        write_delta(&dob[dc + k], &dob[D + dc + k], c * u_im[i], ob[D + dc + k], lr, eps);
      }
    }
    // write s/r deltas with fused AdaGrad
    float* dsb = ds + (int64_t)b * row;
    float* drb = dr + (int64_t)b * row;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= dc) continue;
      write_delta(&dsb[k], &dsb[D + k], a_sre[i], sb[D + k], lr, eps);
      write_delta(&dsb[dc + k], &dsb[D + dc + k], a_sim[i], sb[D + dc + k], lr, eps);
      write_delta(&drb[k], &drb[D + k], a_rre[i], rb[D + k], lr, eps);
      write_delta(&drb[dc + k], &drb[D + dc + k], a_rim[i], rb[D + dc + k], lr, eps);
    }
    if (threadIdx.x == 0) loss[b] = lsum;
  }
}

// softplusf that keeps its relative accuracy where exp(x) is small: there
// 1 + exp(x) rounds the whole term away (softplusf(-30) is 0, not 9.4e-14),
// which shows once a sample's loss has no large term beside it. log1p as its
// series below exp(x) = 0.01, where the next term is under 2.5e-9.
__device__ inline float softplus1pf(float x) {
  if (x > 20.f) return x;
  float t = __expf(x);
  return t < 0.01f ? t * (1.f - t * (0.5f - t * (1.f / 3.f))) : __logf(1.f + t);
}

// The sides step (kernels.h): the positive with N object-side and NS
// subject-side negatives, and gamma * E on the positive's rows. Two passes per
// workgroup. The object pass is k_kge_step's loop (u = s*r fixed) without the
// write of the positive object; s is complete after it and is written there,
// so that the subject pass (v = conj(r)*o fixed, psi = s'.v) holds r, o, v and
// two accumulators, no more rows than the object pass does. r and o are
// written at the end. __launch_bounds__(KT) lets KPT = 8 keep its rows in
// registers.
template <int KPT>
__global__ void __launch_bounds__(KT)
k_kge_step_sides(const float* __restrict__ s, const float* __restrict__ r,
                 const float* __restrict__ o, const float* __restrict__ neg_o,
                 const float* __restrict__ neg_s, float* __restrict__ ds,
                 float* __restrict__ dr, float* __restrict__ do_, float* __restrict__ dneg_o,
                 float* __restrict__ dneg_s, float* __restrict__ loss, int B, int N, int NS,
                 int D, float lr, float eps, float gamma_e, float gamma_r) {
  __shared__ float lds[KT / 64];
  const int dc = D >> 1;
  const int row = D << 1;  // floats per pulled row
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* sb = s + (int64_t)b * row;
    const float* rb = r + (int64_t)b * row;
    const float* pb = o + (int64_t)b * row;

    float r_re[KPT], r_im[KPT], a_rre[KPT], a_rim[KPT];
    float u_re[KPT], u_im[KPT];
    float lsum = 0.f;
    float c0 = 0.f;  // dL/dpsi of the positive
    {
      float s_re[KPT], s_im[KPT], a_sre[KPT], a_sim[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        a_sre[i] = a_sim[i] = a_rre[i] = a_rim[i] = 0.f;
        if (k < dc) {
          s_re[i] = sb[k];
          s_im[i] = sb[dc + k];
          r_re[i] = rb[k];
          r_im[i] = rb[dc + k];
          u_re[i] = s_re[i] * r_re[i] - s_im[i] * r_im[i];
          u_im[i] = s_im[i] * r_re[i] + s_re[i] * r_im[i];
        } else {
          s_re[i] = s_im[i] = r_re[i] = r_im[i] = u_re[i] = u_im[i] = 0.f;
        }
      }

      // object pass: the positive (j = 0), then (s, r, o'_j)
      for (int j = 0; j <= N; ++j) {
        const float* ob = (j == 0) ? pb : neg_o + ((int64_t)b * N + (j - 1)) * row;
        float y = (j == 0) ? 1.f : -1.f;
        float part = 0.f;
        float o_re[KPT], o_im[KPT];
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
          int k = threadIdx.x + i * KT;
          o_re[i] = k < dc ? ob[k] : 0.f;
          o_im[i] = k < dc ? ob[dc + k] : 0.f;
          part += u_re[i] * o_re[i] + u_im[i] * o_im[i];
        }
        float psi = block_reduce_sum(part, lds);
        float c = -y * sigmoidf(-y * psi);  // dL/dpsi, L = softplus(-y*psi)
        if (threadIdx.x == 0) lsum += softplus1pf(-y * psi);
        if (j == 0) c0 = c;

        float* dob = (j == 0) ? nullptr : dneg_o + ((int64_t)b * N + (j - 1)) * row;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
          int k = threadIdx.x + i * KT;
          if (k >= dc) continue;
          a_sre[i] += c * (r_re[i] * o_re[i] + r_im[i] * o_im[i]);
          a_sim[i] += c * (r_re[i] * o_im[i] - r_im[i] * o_re[i]);
          a_rre[i] += c * (s_re[i] * o_re[i] + s_im[i] * o_im[i]);
          a_rim[i] += c * (s_re[i] * o_im[i] - s_im[i] * o_re[i]);
          if (j == 0) continue;  // the positive object waits for the subject pass
          write_delta(&dob[k], &dob[D + k], c * u_re[i], ob[D + k], lr, eps);
          write_delta(&dob[dc + k], &dob[D + dc + k], c * u_im[i], ob[D + dc + k], lr, eps);
        }
      }

      float* dsb = ds + (int64_t)b * row;
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        write_delta(&dsb[k], &dsb[D + k], a_sre[i] + gamma_e * s_re[i], sb[D + k], lr, eps);
        write_delta(&dsb[dc + k], &dsb[D + dc + k], a_sim[i] + gamma_e * s_im[i],
                    sb[D + dc + k], lr, eps);
      }
    }

    // subject pass: (s'_j, r, o)
    float p_re[KPT], p_im[KPT], a_ore[KPT], a_oim[KPT];
    float v_re[KPT], v_im[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      p_re[i] = k < dc ? pb[k] : 0.f;
      p_im[i] = k < dc ? pb[dc + k] : 0.f;
      a_ore[i] = c0 * u_re[i];
      a_oim[i] = c0 * u_im[i];
      v_re[i] = r_re[i] * p_re[i] + r_im[i] * p_im[i];
      v_im[i] = r_re[i] * p_im[i] - r_im[i] * p_re[i];
    }
    for (int j = 0; j < NS; ++j) {
      const float* xb = neg_s + ((int64_t)b * NS + j) * row;
      float* dxb = dneg_s + ((int64_t)b * NS + j) * row;
      float part = 0.f;
      float x_re[KPT], x_im[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        x_re[i] = k < dc ? xb[k] : 0.f;
        x_im[i] = k < dc ? xb[dc + k] : 0.f;
        part += v_re[i] * x_re[i] + v_im[i] * x_im[i];
      }
      float psi = block_reduce_sum(part, lds);
      float c = sigmoidf(psi);  // dL/dpsi, L = softplus(psi)
      if (threadIdx.x == 0) lsum += softplus1pf(psi);
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        a_rre[i] += c * (x_re[i] * p_re[i] + x_im[i] * p_im[i]);
        a_rim[i] += c * (x_re[i] * p_im[i] - x_im[i] * p_re[i]);
        a_ore[i] += c * (x_re[i] * r_re[i] - x_im[i] * r_im[i]);
        a_oim[i] += c * (x_im[i] * r_re[i] + x_re[i] * r_im[i]);
        write_delta(&dxb[k], &dxb[D + k], c * v_re[i], xb[D + k], lr, eps);
        write_delta(&dxb[dc + k], &dxb[D + dc + k], c * v_im[i], xb[D + dc + k], lr, eps);
      }
    }

    float* drb = dr + (int64_t)b * row;
    float* dpb = do_ + (int64_t)b * row;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= dc) continue;
      write_delta(&drb[k], &drb[D + k], a_rre[i] + gamma_r * r_re[i], rb[D + k], lr, eps);
      write_delta(&drb[dc + k], &drb[D + dc + k], a_rim[i] + gamma_r * r_im[i], rb[D + dc + k],
                  lr, eps);
      write_delta(&dpb[k], &dpb[D + k], a_ore[i] + gamma_e * p_re[i], pb[D + k], lr, eps);
      write_delta(&dpb[dc + k], &dpb[D + dc + k], a_oim[i] + gamma_e * p_im[i], pb[D + dc + k],
                  lr, eps);
    }
    if (threadIdx.x == 0) loss[b] = lsum;
  }
}

__global__ void k_kge_score(const float* __restrict__ s, const float* __restrict__ r,
                            const float* __restrict__ cand, float* __restrict__ scores, int B,
                            int E, int D) {
  __shared__ float lds[KT / 64];
  const int dc = D >> 1;
  const int row = D << 1;
  for (int be = blockIdx.x; be < B * E; be += gridDim.x) {
    int b = be / E, e = be % E;
    const float* sb = s + (int64_t)b * row;
    const float* rb = r + (int64_t)b * row;
    const float* ob = cand + (int64_t)e * row;
    float part = 0.f;
    for (int k = threadIdx.x; k < dc; k += KT) {
      float ure = sb[k] * rb[k] - sb[dc + k] * rb[dc + k];
      float uim = sb[dc + k] * rb[k] + sb[k] * rb[dc + k];
      part += ure * ob[k] + uim * ob[dc + k];
    }
    float psi = block_reduce_sum(part, lds);
    if (threadIdx.x == 0) scores[be] = psi;
  }
}

// --------------------------------------------------------------- SGNS

template <int KPT>
__global__ void k_w2v_step(const float* __restrict__ ctr, const float* __restrict__ ctx,
                           const float* __restrict__ neg, float* __restrict__ dctr,
                           float* __restrict__ dctx, float* __restrict__ dneg,
                           float* __restrict__ loss, int B, int N, int D, float lr, float eps) {
  __shared__ float lds[KT / 64];
  const int row = D << 1;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* cb = ctr + (int64_t)b * row;
    float c_emb[KPT], a_c[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      c_emb[i] = k < D ? cb[k] : 0.f;
      a_c[i] = 0.f;
    }

    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      const float* xb = (j == 0) ? ctx + (int64_t)b * row
                                 : neg + ((int64_t)b * N + (j - 1)) * row;
      float y = (j == 0) ? 1.f : -1.f;
      float part = 0.f;
      float x_emb[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        x_emb[i] = k < D ? xb[k] : 0.f;
        part += c_emb[i] * x_emb[i];
      }
      float dot = block_reduce_sum(part, lds);
      float g = -y * sigmoidf(-y * dot);
      if (threadIdx.x == 0) lsum += softplusf(-y * dot);
      float* dxb = (j == 0) ? dctx + (int64_t)b * row
                            : dneg + ((int64_t)b * N + (j - 1)) * row;
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        if (k >= D) continue;
        a_c[i] += g * x_emb[i];
        write_delta(&dxb[k], &dxb[D + k], g * c_emb[i], xb[D + k], lr, eps);
      }
    }
    float* dcb = dctr + (int64_t)b * row;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= D) continue;
      write_delta(&dcb[k], &dcb[D + k], a_c[i], cb[D + k], lr, eps);
    }
    if (threadIdx.x == 0) loss[b] = lsum;
  }
}

// --------------------------------------------------------------- MF

__global__ void k_mf_step(const float* __restrict__ w, const float* __restrict__ h,
                          const float* __restrict__ x, float* __restrict__ dw,
                          float* __restrict__ dh, float* __restrict__ loss, int B, int R,
                          float lr, float lambda, float eps) {
  __shared__ float lds[KT / 64];
  const int row = R << 1;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* wb = w + (int64_t)b * row;
    const float* hb = h + (int64_t)b * row;
    float part = 0.f;
    for (int k = threadIdx.x; k < R; k += KT) part += wb[k] * hb[k];
    float pred = block_reduce_sum(part, lds);
    float e = x[b] - pred;
    if (threadIdx.x == 0) loss[b] = e * e;
    float* dwb = dw + (int64_t)b * row;
    float* dhb = dh + (int64_t)b * row;
    for (int k = threadIdx.x; k < R; k += KT) {
      float gw = -2.f * e * hb[k] + 2.f * lambda * wb[k];
      float gh = -2.f * e * wb[k] + 2.f * lambda * hb[k];
      write_delta(&dwb[k], &dwb[R + k], gw, wb[R + k], lr, eps);
      write_delta(&dhb[k], &dhb[R + k], gh, hb[R + k], lr, eps);
    }
  }
}

// --------------------------------------------------------------- MF loss

// The two sums are kept in double from the first sample on: up to 16384
// workgroups add their share with one atomic each, in any order, and an fp32
// sum of that many terms drifts by up to 2e-6 of the total, run to run. The
// per-sample terms stay fp32.
__global__ void k_mf_loss(const float* __restrict__ w, const float* __restrict__ h,
                          const float* __restrict__ x, double* __restrict__ acc2, int B, int R,
                          float lambda) {
  __shared__ float lds[2][KT / 64];
  const int row = R << 1;
  double se = 0.0, reg = 0.0;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* wb = w + (int64_t)b * row;
    const float* hb = h + (int64_t)b * row;
    float part = 0.f, nrm = 0.f;
    for (int k = threadIdx.x; k < R; k += KT) {
      float wv = wb[k], hv = hb[k];
      part += wv * hv;
      nrm += wv * wv + hv * hv;
    }
    float pred = block_reduce_sum(part, lds[0]);
    float n2 = block_reduce_sum(nrm, lds[1]);
    if (threadIdx.x == 0) {
      float e = x[b] - pred;
      se += (double)(e * e);
      reg += (double)(lambda * n2);
    }
  }
  if (threadIdx.x == 0) {
    atomicAdd(&acc2[0], se);
    atomicAdd(&acc2[1], reg);
  }
}

void mf_loss_gpu(const float* w, const float* h, const float* x, double* acc2, int B, int R,
                 float lambda, void* stream) {
  if (B < 1) return;
  hipLaunchKernelGGL(k_mf_loss, dim3(grid_for(B)), dim3(KT), 0, (hipStream_t)stream, w, h, x,
                     acc2, B, R, lambda);
}

// --------------------------------------------------------------- alias draw

__device__ __host__ inline uint64_t pcg_hash64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

__global__ void k_alias_draw(const float* __restrict__ prob, const int32_t* __restrict__ alias,
                             int64_t n, uint64_t seed, int64_t N, int64_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < N; i += stride) {
    uint64_t h = pcg_hash64(seed ^ (uint64_t)i * 0x9e3779b97f4a7c15ULL);
    int64_t slot = (int64_t)(h % (uint64_t)n);
    float u = (float)((h >> 40) & 0xffffff) * (1.0f / 16777216.0f);
    out[i] = (u < prob[slot]) ? slot : (int64_t)alias[slot];
  }
}

// --------------------------------------------------------------- launchers

void kge_complex_step_gpu(const float* s, const float* r, const float* o, const float* neg,
                          float* ds, float* dr, float* do_, float* dneg, float* loss, int B,
                          int N, int D, float lr, float eps, void* stream) {
  dispatch_kpt(D >> 1, [&](auto kpt) {
    hipLaunchKernelGGL(k_kge_step<decltype(kpt)::value>, dim3(grid_for(B)), dim3(KT), 0,
                       (hipStream_t)stream, s, r, o, neg, ds, dr, do_, dneg, loss, B, N, D, lr,
                       eps);
  });
}
void kge_complex_step_sides_gpu(const float* s, const float* r, const float* o,
                                const float* neg_o, const float* neg_s, float* ds, float* dr,
                                float* do_, float* dneg_o, float* dneg_s, float* loss, int B,
                                int N, int NS, int D, float lr, float eps, float gamma_e,
                                float gamma_r, void* stream) {
  if (B < 1) return;
  // No subject side and no regulariser is the one-sided step, and is run by
  // its kernel: the two kernels' object passes are the same expressions in the
  // same order, but the compiler contracts them differently (acc + g*g is an
  // fma in one and a mul and an add in the other), so only the same code
  // gives the same bits.
  if (NS == 0 && gamma_e == 0.f && gamma_r == 0.f)
    return kge_complex_step_gpu(s, r, o, neg_o, ds, dr, do_, dneg_o, loss, B, N, D, lr, eps,
                                stream);
  dispatch_kpt(D >> 1, [&](auto kpt) {
    hipLaunchKernelGGL(k_kge_step_sides<decltype(kpt)::value>, dim3(grid_for(B)), dim3(KT), 0,
                       (hipStream_t)stream, s, r, o, neg_o, neg_s, ds, dr, do_, dneg_o, dneg_s,
                       loss, B, N, NS, D, lr, eps, gamma_e, gamma_r);
  });
}
void kge_complex_score_gpu(const float* s, const float* r, const float* cand, float* scores,
                           int B, int E, int D, void* stream) {
  hipLaunchKernelGGL(k_kge_score, dim3(grid_for((int64_t)B * E)), dim3(KT), 0,
                     (hipStream_t)stream, s, r, cand, scores, B, E, D);
}
void w2v_sgns_step_gpu(const float* ctr, const float* ctx, const float* neg, float* dctr,
                       float* dctx, float* dneg, float* loss, int B, int N, int D, float lr,
                       float eps, void* stream) {
  dispatch_kpt(D, [&](auto kpt) {
    hipLaunchKernelGGL(k_w2v_step<decltype(kpt)::value>, dim3(grid_for(B)), dim3(KT), 0,
                       (hipStream_t)stream, ctr, ctx, neg, dctr, dctx, dneg, loss, B, N, D, lr,
                       eps);
  });
}
void mf_update_step_gpu(const float* w, const float* h, const float* x, float* dw, float* dh,
                        float* loss, int B, int R, float lr, float lambda, float eps,
                        void* stream) {
  hipLaunchKernelGGL(k_mf_step, dim3(grid_for(B)), dim3(KT), 0, (hipStream_t)stream, w, h, x, dw,
                     dh, loss, B, R, lr, lambda, eps);
}

}  // namespace adapm

namespace adapm {
void alias_draw_gpu(const float* prob, const int32_t* alias, int64_t n, uint64_t seed,
                    int64_t N, int64_t* out, void* stream) {
  if (N == 0) return;
  hipLaunchKernelGGL(k_alias_draw, dim3(grid_for((N + 255) / 256, 4096)), dim3(256), 0,
                     (hipStream_t)stream, prob, alias, n, seed, N, out);
}
}  // namespace adapm

// --------------------------------------------------------------- uniform draw
//
// numpy-exact uniform keys (ustream.h) in two launches: generate + flag,
// then compact. The state is written back by the one thread of the second
// launch that can: the thread that writes key n-1 knows how many words were
// consumed; if the words fall short of n keys nobody writes key n-1, and
// thread 0 of the last workgroup, which has the total, continues the
// stream. Either needs nothing from another workgroup of its launch, so
// there is no fence and no third launch. One thread per chunk of USTREAM_CHUNK
// words, USTREAM_BLOCK chunks per workgroup; the scratch keys of a
// workgroup are interleaved by thread (word i of thread t at i*KT + t), so
// both launches touch them with coalesced accesses. The 2 MB of scratch at
// the benchmark's 262,144 draws stay in L2 between the launches.
namespace adapm {

static_assert(USTREAM_BLOCK == KT, "one chunk per thread of a KT workgroup");

__device__ inline int64_t block_reduce_i64(int64_t v, int64_t* lds) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t out = 0;
  for (int i = 0; i < KT / 64; ++i) out += lds[i];
  __syncthreads();
  return out;
}

template <typename T>
__device__ inline T* ustream_block_keys(T* tmp, int64_t nb, int64_t block) {
  return tmp + USTREAM_TMP_COUNTS + nb + block * (KT * USTREAM_CHUNK) + threadIdx.x;
}

__global__ void __launch_bounds__(KT)
k_ustream_gen(const uint64_t* __restrict__ state, UStreamRange r, int64_t words, int64_t chunks,
              int64_t* __restrict__ tmp, int64_t nb) {
  __shared__ int64_t lds[KT / 64];
  const int64_t c = (int64_t)blockIdx.x * KT + threadIdx.x;
  int64_t cnt = 0;
  if (c < chunks)
    cnt = ustream_gen_chunk(state, r, words, c, ustream_block_keys(tmp, nb, blockIdx.x), KT);
  cnt = block_reduce_i64(cnt, lds);
  if (threadIdx.x == 0) {
    tmp[USTREAM_TMP_COUNTS + blockIdx.x] = cnt;
  }
}

__global__ void __launch_bounds__(KT)
k_ustream_compact(uint64_t* __restrict__ state, UStreamRange r, int64_t n, int64_t words,
                  int64_t chunks, const int64_t* __restrict__ tmp, int64_t nb,
                  int64_t* __restrict__ out) {
  __shared__ int64_t lds[KT / 64];
  __shared__ int wave_tot[KT / 64];
  const int64_t* counts = tmp + USTREAM_TMP_COUNTS;
  int64_t part = 0;
  for (int64_t i = threadIdx.x; i < (int64_t)blockIdx.x; i += KT) part += counts[i];
  const int64_t off = block_reduce_i64(part, lds);
  const int64_t c = (int64_t)blockIdx.x * KT + threadIdx.x;
  const bool live = off < n && c < chunks;  // off is uniform over the workgroup
  const int64_t* kc = ustream_block_keys(tmp, nb, blockIdx.x);
  int64_t k[USTREAM_CHUNK];
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < USTREAM_CHUNK; ++i) {
    k[i] = live ? kc[i * KT] : USTREAM_REJECTED;
    cnt += (k[i] != USTREAM_REJECTED);
  }
  // exclusive scan of cnt over the workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = cnt;
  for (int d = 1; d < 64; d <<= 1) {
    int y = __shfl_up(incl, d, 64);
    if (lane >= d) incl += y;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  int64_t idx = off + incl - cnt;
  for (int i = 0; i < wave; ++i) idx += wave_tot[i];
  int64_t consumed = 0;
#pragma unroll
  for (int i = 0; i < USTREAM_CHUNK; ++i) {
    if (k[i] == USTREAM_REJECTED) continue;
    if (idx < n) {
      out[idx] = k[i];
      if (idx == n - 1) consumed = c * USTREAM_CHUNK + i + 1;
    }
    ++idx;
  }
  if (consumed) {
    ustream_finish(state, r, n, words, n, consumed, out);
  } else if (blockIdx.x == nb - 1 && threadIdx.x == 0) {
    int64_t total = off;
    for (int i = 0; i < KT / 64; ++i) total += wave_tot[i];
    if (total < n) ustream_finish(state, r, n, words, total, 0, out);
  }
}

void uniform_draw_gpu(uint64_t* state, int64_t lo, uint32_t excl, uint32_t thr, int64_t n,
                      int64_t words, int64_t* out, int64_t* tmp, void* stream) {
  if (n <= 0) return;
  const UStreamRange r{lo, excl, thr};
  const int64_t chunks = ustream_chunks(words), nb = ustream_blocks(words);
  auto st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ustream_gen, dim3((unsigned)nb), dim3(KT), 0, st, state, r, words, chunks,
                     tmp, nb);
  hipLaunchKernelGGL(k_ustream_compact, dim3((unsigned)nb), dim3(KT), 0, st, state, r, n, words,
                     chunks, tmp, nb, out);
}

__global__ void k_copy_keys(int64_t* __restrict__ dst, const int64_t* __restrict__ src,
                            int64_t n) {
  int64_t i = (int64_t)blockIdx.x * KT + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

bool copy_keys_gpu(int64_t* dst, const int64_t* src_host, int64_t n, void* stream) {
  if (n <= 0) return true;
  void* src = nullptr;  // fails for memory the device cannot read
  if (hipHostGetDevicePointer(&src, const_cast<int64_t*>(src_host), 0) != hipSuccess || !src) {
    (void)hipGetLastError();
    return false;
  }
  hipLaunchKernelGGL(k_copy_keys, dim3((unsigned)((n + KT - 1) / KT)), dim3(KT), 0,
                     (hipStream_t)stream, dst, static_cast<const int64_t*>(src), n);
  return true;
}
}  // namespace adapm

namespace adapm {

// RESCAL step: one workgroup per positive triple; R staged in LDS
// (dim <= 128 -> 64 KiB). See kernels.h for the math factorization.
__global__ void k_rescal_step(const float* __restrict__ s, const float* __restrict__ r,
                              const float* __restrict__ o, const float* __restrict__ neg,
                              float* __restrict__ ds, float* __restrict__ drl,
                              float* __restrict__ do_, float* __restrict__ dneg,
                              float* __restrict__ loss, int B, int N, int D, float lr,
                              float eps) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Rm = smem;            // D*D
  float* u = Rm + D * D;       // D
  float* w = u + D;            // D
  float* es = w + D;           // D
  float* red = es + D;         // KT/64 reduction scratch
  const int erow = 2 * D;
  const int64_t rrow = 2LL * D * D;

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* sb = s + (int64_t)b * erow;
    const float* rb = r + (int64_t)b * rrow;
    for (int i = threadIdx.x; i < D * D; i += KT) Rm[i] = rb[i];
    for (int i = threadIdx.x; i < D; i += KT) {
      es[i] = sb[i];
      w[i] = 0.f;
    }
    __syncthreads();
    // u = R^T e_s: thread j computes column j
    for (int j = threadIdx.x; j < D; j += KT) {
      float a = 0.f;
      for (int i = 0; i < D; ++i) a += Rm[i * D + j] * es[i];
      u[j] = a;
    }
    __syncthreads();

    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      const float* ob = (j == 0) ? o + (int64_t)b * erow
                                 : neg + ((int64_t)b * N + j - 1) * erow;
      float* dob = (j == 0) ? do_ + (int64_t)b * erow
                            : dneg + ((int64_t)b * N + j - 1) * erow;
      float y = (j == 0) ? 1.f : -1.f;
      float part = 0.f;
      for (int k = threadIdx.x; k < D; k += KT) part += u[k] * ob[k];
      float dot = block_reduce_sum(part, red);
      float c = -y * sigmoidf(-y * dot);
      if (threadIdx.x == 0) lsum += softplusf(-y * dot);
      for (int k = threadIdx.x; k < D; k += KT) {
        w[k] += c * ob[k];  // single writer per k: thread-private index
        write_delta(&dob[k], &dob[D + k], c * u[k], ob[D + k], lr, eps);
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) loss[b] = lsum;

    // de_s = R w
    float* dsb = ds + (int64_t)b * erow;
    for (int i = threadIdx.x; i < D; i += KT) {
      float a = 0.f;
      for (int k = 0; k < D; ++k) a += Rm[i * D + k] * w[k];
      write_delta(&dsb[i], &dsb[D + i], a, sb[D + i], lr, eps);
    }
    // dR = e_s w^T
    float* drb = drl + (int64_t)b * rrow;
    for (int idx = threadIdx.x; idx < D * D; idx += KT) {
      int i = idx / D, k = idx % D;
      const int64_t acc = (int64_t)D * D + idx;
      write_delta(&drb[idx], &drb[acc], es[i] * w[k], rb[acc], lr, eps);
    }
    __syncthreads();
  }
}

void rescal_step_gpu(const float* s, const float* r, const float* o, const float* neg,
                     float* ds, float* drl, float* do_, float* dneg, float* loss, int B, int N,
                     int D, float lr, float eps, void* stream) {
  size_t smem = (size_t)(D * D + 3 * D + KT / 64) * sizeof(float);
  if (B < 1) return;
  hipLaunchKernelGGL(k_rescal_step, dim3(grid_for(B, 8192)), dim3(KT), smem, (hipStream_t)stream,
                     s, r, o, neg, ds, drl, do_, dneg, loss, B, N, D, lr, eps);
}

// RESCAL sides step (kernels.h): k_rescal_step's shape, one workgroup per
// positive with R in LDS, and beside R the six D-vectors u = R^T s, w, e_s,
// v = R o, z, e_o. The object pass fills w and writes the o'_j, the subject
// pass fills z and writes the s'_j; the positive's s, o and R are written
// after both, since o's gradient needs z.
__global__ void __launch_bounds__(KT)
k_rescal_step_sides(const float* __restrict__ s, const float* __restrict__ r,
                    const float* __restrict__ o, const float* __restrict__ neg_o,
                    const float* __restrict__ neg_s, float* __restrict__ ds,
                    float* __restrict__ drl, float* __restrict__ do_,
                    float* __restrict__ dneg_o, float* __restrict__ dneg_s,
                    float* __restrict__ loss, int B, int N, int NS, int D, float lr, float eps,
                    float gamma_e, float gamma_r) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Rm = smem;            // D*D
  float* u = Rm + D * D;       // D
  float* w = u + D;            // D
  float* es = w + D;           // D
  float* v = es + D;           // D
  float* z = v + D;            // D
  float* eo = z + D;           // D
  float* red = eo + D;         // KT/64 reduction scratch
  const int erow = 2 * D;
  const int64_t rrow = 2LL * D * D;

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* sb = s + (int64_t)b * erow;
    const float* rb = r + (int64_t)b * rrow;
    const float* pb = o + (int64_t)b * erow;
    for (int i = threadIdx.x; i < D * D; i += KT) Rm[i] = rb[i];
    for (int i = threadIdx.x; i < D; i += KT) {
      es[i] = sb[i];
      eo[i] = pb[i];
      w[i] = 0.f;
      z[i] = 0.f;
    }
    __syncthreads();
    // u = R^T e_s (thread j: column j), v = R e_o (thread j: row j)
    for (int j = threadIdx.x; j < D; j += KT) {
      float a = 0.f, c = 0.f;
      for (int i = 0; i < D; ++i) {
        a += Rm[i * D + j] * es[i];
        c += Rm[j * D + i] * eo[i];
      }
      u[j] = a;
      v[j] = c;
    }
    __syncthreads();

    float lsum = 0.f;
    float c0 = 0.f;  // dL/dpsi of the positive
    // object pass: the positive (j = 0), then (s, R, o'_j)
    for (int j = 0; j <= N; ++j) {
      const float* ob = (j == 0) ? pb : neg_o + ((int64_t)b * N + j - 1) * erow;
      float y = (j == 0) ? 1.f : -1.f;
      float part = 0.f;
      for (int k = threadIdx.x; k < D; k += KT) part += u[k] * ob[k];
      float dot = block_reduce_sum(part, red);
      float c = -y * sigmoidf(-y * dot);
      if (threadIdx.x == 0) lsum += softplus1pf(-y * dot);
      if (j == 0) {  // the positive object waits for the subject pass
        c0 = c;
        for (int k = threadIdx.x; k < D; k += KT) w[k] += c * ob[k];
        continue;
      }
      float* dob = dneg_o + ((int64_t)b * N + j - 1) * erow;
      for (int k = threadIdx.x; k < D; k += KT) {
        w[k] += c * ob[k];  // single writer per k: thread-private index
        write_delta(&dob[k], &dob[D + k], c * u[k], ob[D + k], lr, eps);
      }
    }
    // subject pass: (s'_j, R, o)
    for (int j = 0; j < NS; ++j) {
      const float* xb = neg_s + ((int64_t)b * NS + j) * erow;
      float* dxb = dneg_s + ((int64_t)b * NS + j) * erow;
      float part = 0.f;
      for (int k = threadIdx.x; k < D; k += KT) part += v[k] * xb[k];
      float dot = block_reduce_sum(part, red);
      float a = sigmoidf(dot);
      if (threadIdx.x == 0) lsum += softplus1pf(dot);
      for (int k = threadIdx.x; k < D; k += KT) {
        z[k] += a * xb[k];
        write_delta(&dxb[k], &dxb[D + k], a * v[k], xb[D + k], lr, eps);
      }
    }
    if (threadIdx.x == 0) loss[b] = lsum;
    __syncthreads();  // w and z complete

    // de_s = R w + gamma_e e_s, de_o = c0 u + R^T z + gamma_e e_o
    float* dsb = ds + (int64_t)b * erow;
    float* dpb = do_ + (int64_t)b * erow;
    for (int i = threadIdx.x; i < D; i += KT) {
      float a = 0.f, c = 0.f;
      for (int k = 0; k < D; ++k) {
        a += Rm[i * D + k] * w[k];
        c += Rm[k * D + i] * z[k];
      }
      write_delta(&dsb[i], &dsb[D + i], a + gamma_e * es[i], sb[D + i], lr, eps);
      write_delta(&dpb[i], &dpb[D + i], c0 * u[i] + c + gamma_e * eo[i], pb[D + i], lr, eps);
    }
    // dR = e_s w^T + z e_o^T + gamma_r R
    float* drb = drl + (int64_t)b * rrow;
    for (int idx = threadIdx.x; idx < D * D; idx += KT) {
      int i = idx / D, k = idx % D;
      const int64_t acc = (int64_t)D * D + idx;
      write_delta(&drb[idx], &drb[acc], es[i] * w[k] + z[i] * eo[k] + gamma_r * Rm[idx],
                  rb[acc], lr, eps);
    }
    __syncthreads();
  }
}

// floats of LDS k_rescal_step_sides uses at dimension D: R, six D-vectors
// and the reduction scratch (158,384 B at D = 196, of 163,840 B a workgroup
// may declare)
static inline size_t rescal_sides_lds_bytes(int D) {
  return ((size_t)D * D + 6 * (size_t)D + KT / 64) * sizeof(float);
}

void rescal_step_sides_gpu(const float* s, const float* r, const float* o, const float* neg_o,
                           const float* neg_s, float* ds, float* drl, float* do_,
                           float* dneg_o, float* dneg_s, float* loss, int B, int N, int NS,
                           int D, float lr, float eps, float gamma_e, float gamma_r,
                           void* stream) {
  if (B < 1) return;
  hipLaunchKernelGGL(k_rescal_step_sides, dim3(grid_for(B, 8192)), dim3(KT),
                     rescal_sides_lds_bytes(D), (hipStream_t)stream, s, r, o, neg_o, neg_s, ds,
                     drl, do_, dneg_o, dneg_s, loss, B, N, NS, D, lr, eps, gamma_e, gamma_r);
}

}  // namespace adapm

namespace adapm {

// Row resolution for the fused slab-direct kernels. world >= 1: identity
// layout, key k lives at (k/world)*plen (the world==1 single-rank fast
// path with zero host work). world == 0: the "keys" arrays carry
// precomputed float OFFSETS into the slab (the world>1 / relocated-layout
// path: the host metadata pass resolves each key's slot and compacts
// all-local samples; remote ones go through the classic pull/push path).
__device__ inline float* row_at(float* slab, int64_t v, int32_t plen, int world) {
  return world ? slab + (v / world) * (int64_t)plen : slab + v;
}

// ---- per-launch row tags (see kernels.h): one word per slab row. Every
// store below is a plain store of a whole word; none of the passes holds a
// read-modify-write.
__device__ inline int64_t rowtag_key(const RowTagKeys& ks, int64_t i) {
  // occurrence i of the concatenated key arrays
  int a = 0;
  while (a < ks.count - 1 && i >= ks.n[a]) {
    i -= ks.n[a];
    ++a;
  }
  return ks.keys[a][i];
}

// tag pass, occurrence i: whoever stores last owns the row
__device__ inline void rowtag_tag(uint32_t* tags, int64_t row, int64_t i) {
  tags[row] = (uint32_t)i;
}

// flag pass, occurrence i: a tag that is not mine means the row has a
// second occurrence (its owner's index, or ROWTAG_SHARED already)
__device__ inline void rowtag_flag(uint32_t* tags, int64_t row, int64_t i) {
  if (tags[row] != (uint32_t)i) tags[row] = ROWTAG_SHARED;
}

// Tag pass fused with the key upload: see keys_land_gpu in kernels.h.
__global__ void k_keys_land(uint32_t* __restrict__ tags, int64_t* __restrict__ dst,
                            const int64_t* __restrict__ src, int64_t n_copy,
                            const int64_t* __restrict__ dev_keys, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * KT + threadIdx.x;
  if (i >= total) return;
  int64_t row;
  if (i < n_copy) {
    row = src[i];
    dst[i] = row;
  } else {
    row = dev_keys[i - n_copy];
  }
  rowtag_tag(tags, row, i);
}

// the tag pass alone, over keys that are already on the device
__global__ void k_rowtag_tag(uint32_t* __restrict__ tags, RowTagKeys ks, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * KT + threadIdx.x;
  if (i >= total) return;
  rowtag_tag(tags, rowtag_key(ks, i), i);
}

__global__ void k_rowtag_flag(uint32_t* __restrict__ tags, RowTagKeys ks, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * KT + threadIdx.x;
  if (i >= total) return;
  rowtag_flag(tags, rowtag_key(ks, i), i);
}

// bits pass, occurrence i: rewrite the whole bitmap word of its row from the
// 32 tags behind it (one aligned 128-byte line). Every writer of a word
// stores the same value, because the tags no longer change. Tags of rows
// that are not in the batch are stale; so are their bits, which nobody reads.
__global__ void k_rowtag_bits(const uint32_t* __restrict__ tags, uint32_t* __restrict__ bits,
                              RowTagKeys ks, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * KT + threadIdx.x;
  if (i >= total) return;
  const int64_t w = rowtag_key(ks, i) >> 5;
  const uint4* t = reinterpret_cast<const uint4*>(tags + (w << 5));
  uint32_t word = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint4 v = t[q];
    word |= ((uint32_t)(v.x == ROWTAG_SHARED) | (uint32_t)(v.y == ROWTAG_SHARED) << 1 |
             (uint32_t)(v.z == ROWTAG_SHARED) << 2 | (uint32_t)(v.w == ROWTAG_SHARED) << 3)
            << (4 * q);
  }
  bits[w] = word;
}

static int64_t rowtag_total(const RowTagKeys& ks) {
  int64_t total = 0;
  for (int a = 0; a < ks.count; ++a) total += ks.n[a];
  return total;
}

void rowtag_tag_gpu(uint32_t* tags, const RowTagKeys& ks, void* stream) {
  const int64_t total = rowtag_total(ks);
  if (total == 0) return;
  hipLaunchKernelGGL(k_rowtag_tag, dim3((unsigned)((total + KT - 1) / KT)), dim3(KT), 0,
                     (hipStream_t)stream, tags, ks, total);
}

void rowtag_flag_gpu(uint32_t* tags, const RowTagKeys& ks, void* stream) {
  const int64_t total = rowtag_total(ks);
  if (total == 0) return;
  hipLaunchKernelGGL(k_rowtag_flag, dim3((unsigned)((total + KT - 1) / KT)), dim3(KT), 0,
                     (hipStream_t)stream, tags, ks, total);
}

void rowtag_bits_gpu(const uint32_t* tags, uint32_t* bits, const RowTagKeys& ks, void* stream) {
  const int64_t total = rowtag_total(ks);
  if (total == 0) return;
  hipLaunchKernelGGL(k_rowtag_bits, dim3((unsigned)((total + KT - 1) / KT)), dim3(KT), 0,
                     (hipStream_t)stream, tags, bits, ks, total);
}

bool keys_land_gpu(uint32_t* tags, int64_t* dst, const int64_t* src_host, int64_t n_copy,
                   const int64_t* dev_keys, int64_t n_dev, void* stream) {
  const int64_t total = n_copy + n_dev;
  if (total <= 0) return true;
  void* src = nullptr;  // fails for memory the device cannot read
  if (n_copy > 0 &&
      (hipHostGetDevicePointer(&src, const_cast<int64_t*>(src_host), 0) != hipSuccess || !src)) {
    (void)hipGetLastError();
    return false;
  }
  hipLaunchKernelGGL(k_keys_land, dim3((unsigned)((total + KT - 1) / KT)), dim3(KT), 0,
                     (hipStream_t)stream, tags, dst, static_cast<const int64_t*>(src), n_copy,
                     dev_keys, total);
  return true;
}

// UNIQ: is the row shared with another occurrence of this batch? The word
// address depends only on the key, so this load runs beside the row loads
// and is uniform across the block. It reads the bitmap and not the tags:
// the load is a scalar one whose latency the block waits out, and the
// bitmap (1.25 MB at 10M keys) stays in cache where the tags (40 MB) do not.
template <bool UNIQ>
__device__ inline bool row_shared(const uint32_t* __restrict__ bits, int64_t key) {
  if (!UNIQ) return true;
  return (bits[key >> 5] >> (int)(key & 31)) & 1u;
}

// row = row + delta with a plain store, rounded exactly like the atomic it
// replaces: the add must not be contracted into an fma with the multiply
// that produced delta.
__device__ inline float plain_add(float a, float delta) {
#pragma clang fp contract(off)
  return a + delta;
}

// Fused kernels: one lane's AdaGrad update applied to the slab row itself,
// *p_emb += delta and *p_acc += g^2. A row shared with another occurrence
// of the batch takes atomics; the only writer of a row stores over the
// values (emb, acc) it read. The SGNS and MF steps have no row tags and
// pass shared = true.
__device__ inline void slab_adagrad(float* p_emb, float* p_acc, float g, float emb, float acc,
                                    float lr, float eps, bool shared) {
  float d = adagrad_delta(g, acc, lr, eps);
  if (shared) {
    atomicAdd(p_emb, d);
    atomicAdd(p_acc, g * g);
  } else {
    *p_emb = plain_add(emb, d);
    *p_acc = plain_add(acc, g * g);
  }
}

// slab_adagrad for a complex lane (re at k, im at dc + k) of the fused ComplEx
// step, both halves under one branch. A macro on purpose, and the only one:
// the KPT = 8 instantiations of k_kge_step_fused spill, and their register
// allocation is so sensitive that moving these statements into an inlined
// function (even just calling adagrad_delta here) adds 44-120 bytes of
// scratch per lane and 15-17% to the D = 4096 step
// (profiles/fused_skeleton_stats.txt). Expands in a scope with k, dc, D, lr,
// eps.
#define SLAB_ADAGRAD_COMPLEX(row, shared, g_re, g_im, emb_re, emb_im, acc_re, acc_im) \
  do {                                                                                \
    float G_re = (acc_re) + (g_re) * (g_re);                                          \
    float G_im = (acc_im) + (g_im) * (g_im);                                          \
    float d_re = -lr * (g_re) * __frsqrt_rn(G_re + eps);                              \
    float d_im = -lr * (g_im) * __frsqrt_rn(G_im + eps);                              \
    if (shared) {                                                                     \
      atomicAdd(&(row)[k], d_re);                                                     \
      atomicAdd(&(row)[dc + k], d_im);                                                \
      atomicAdd(&(row)[D + k], (g_re) * (g_re));                                      \
      atomicAdd(&(row)[D + dc + k], (g_im) * (g_im));                                 \
    } else {                                                                          \
      (row)[k] = plain_add(emb_re, d_re);                                             \
      (row)[dc + k] = plain_add(emb_im, d_im);                                        \
      (row)[D + k] = plain_add(acc_re, (g_re) * (g_re));                              \
      (row)[D + dc + k] = plain_add(acc_im, (g_im) * (g_im));                         \
    }                                                                                 \
  } while (0)

// Fused ComplEx step — see kernels.h. Structure mirrors k_kge_step but
// rows come from / return to the slab itself. UNIQ = false is the
// all-atomic kernel (bits unused); UNIQ = true writes the rows that the
// row tags' `bits` show to be unique in this batch with plain stores.
template <int KPT, bool UNIQ>
__global__ void k_kge_step_fused(float* __restrict__ slab, const int64_t* __restrict__ keys_s,
                                 const int64_t* __restrict__ keys_r,
                                 const int64_t* __restrict__ keys_o,
                                 const int64_t* __restrict__ keys_neg, float* __restrict__ loss,
                                 int B, int N, int D, int32_t plen, int world, float lr,
                                 float eps, const uint32_t* __restrict__ bits,
                                 unsigned long long* __restrict__ shared_stat) {
  __shared__ float lds[KT / 64];
  const int dc = D >> 1;
  // the bits imply the single-rank layout: a constant spares row_at the
  // 64-bit division
  const int w = UNIQ ? 1 : world;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t key_s = keys_s[b], key_r = keys_r[b];
    const float* sb = row_at(slab, key_s, plen, w);
    const float* rb = row_at(slab, key_r, plen, w);
    const bool s_shared = row_shared<UNIQ>(bits, key_s);
    const bool r_shared = row_shared<UNIQ>(bits, key_r);
    unsigned n_shared = (unsigned)s_shared + (unsigned)r_shared;

    float s_re[KPT], s_im[KPT], r_re[KPT], r_im[KPT];
    float a_sre[KPT], a_sim[KPT], a_rre[KPT], a_rim[KPT];
    float u_re[KPT], u_im[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      a_sre[i] = a_sim[i] = a_rre[i] = a_rim[i] = 0.f;
      if (k < dc) {
        s_re[i] = sb[k];
        s_im[i] = sb[dc + k];
        r_re[i] = rb[k];
        r_im[i] = rb[dc + k];
        u_re[i] = s_re[i] * r_re[i] - s_im[i] * r_im[i];
        u_im[i] = s_im[i] * r_re[i] + s_re[i] * r_im[i];
      } else {
        s_re[i] = s_im[i] = r_re[i] = r_im[i] = u_re[i] = u_im[i] = 0.f;
      }
    }

    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      int64_t ok = (j == 0) ? keys_o[b] : keys_neg[(int64_t)b * N + (j - 1)];
      float* ob = row_at(slab, ok, plen, w);
      const bool o_shared = row_shared<UNIQ>(bits, ok);
      n_shared += (unsigned)o_shared;
      float y = (j == 0) ? 1.f : -1.f;
      float part = 0.f;
      float o_re[KPT], o_im[KPT], Go_re[KPT], Go_im[KPT];
      // accumulator halves ride with the embedding halves, so their
      // latency hides behind the block reduction
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        o_re[i] = k < dc ? ob[k] : 0.f;
        o_im[i] = k < dc ? ob[dc + k] : 0.f;
        Go_re[i] = k < dc ? ob[D + k] : 0.f;
        Go_im[i] = k < dc ? ob[D + dc + k] : 0.f;
        part += u_re[i] * o_re[i] + u_im[i] * o_im[i];
      }
      float psi = block_reduce_sum(part, lds);
      float c = -y * sigmoidf(-y * psi);
      if (threadIdx.x == 0) lsum += softplusf(-y * psi);

#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        a_sre[i] += c * (r_re[i] * o_re[i] + r_im[i] * o_im[i]);
        a_sim[i] += c * (r_re[i] * o_im[i] - r_im[i] * o_re[i]);
        a_rre[i] += c * (s_re[i] * o_re[i] + s_im[i] * o_im[i]);
        a_rim[i] += c * (s_re[i] * o_im[i] - s_im[i] * o_re[i]);
        float g_re = c * u_re[i];
        float g_im = c * u_im[i];
        SLAB_ADAGRAD_COMPLEX(ob, o_shared, g_re, g_im, o_re[i], o_im[i], Go_re[i], Go_im[i]);
      }
    }
    float* dsb = const_cast<float*>(sb);
    float* drb = const_cast<float*>(rb);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= dc) continue;
      float Gs_re = sb[D + k], Gs_im = sb[D + dc + k];
      SLAB_ADAGRAD_COMPLEX(dsb, s_shared, a_sre[i], a_sim[i], s_re[i], s_im[i], Gs_re, Gs_im);
      float Gr_re = rb[D + k], Gr_im = rb[D + dc + k];
      SLAB_ADAGRAD_COMPLEX(drb, r_shared, a_rre[i], a_rim[i], r_re[i], r_im[i], Gr_re, Gr_im);
    }
    if (threadIdx.x == 0) {
      loss[b] = lsum;
      if (UNIQ && shared_stat) atomicAdd(shared_stat, (unsigned long long)n_shared);
    }
  }
}

#undef SLAB_ADAGRAD_COMPLEX

void kge_complex_step_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                const int64_t* keys_o, const int64_t* keys_neg, float* loss,
                                int B, int N, int D, int32_t plen, int world, float lr,
                                float eps, void* stream, const uint32_t* bits,
                                unsigned long long* shared_stat) {
  if (B < 1) return;  // unlike the other steps, an empty batch enqueues nothing
  // bits are indexed by key, which is the row only in the single-rank
  // identity layout; every other addressing mode stays all-atomic
  const bool uniq = bits != nullptr && world == 1;
  if (!uniq) bits = nullptr, shared_stat = nullptr;
  dispatch_kpt(D >> 1, [&](auto kpt) {
    constexpr int KPT = decltype(kpt)::value;
    hipLaunchKernelGGL((uniq ? k_kge_step_fused<KPT, true> : k_kge_step_fused<KPT, false>),
                       dim3(grid_for(B)), dim3(KT), 0, (hipStream_t)stream, slab, keys_s, keys_r,
                       keys_o, keys_neg, loss, B, N, D, plen, world, lr, eps, bits,
                       shared_stat);
  });
}

// One complex lane (re at k, im at dc + k) of a slab row through slab_adagrad.
__device__ inline void slab_adagrad_complex(float* row, int k, int dc, int D, float g_re,
                                            float g_im, float emb_re, float emb_im, float acc_re,
                                            float acc_im, float lr, float eps, bool shared) {
  slab_adagrad(&row[k], &row[D + k], g_re, emb_re, acc_re, lr, eps, shared);
  slab_adagrad(&row[dc + k], &row[D + dc + k], g_im, emb_im, acc_im, lr, eps, shared);
}

// Fused sides step: k_kge_step_sides on the slab's own rows, with the
// addressing and the UNIQ / bits contract of k_kge_step_fused. Every row is
// written once per occurrence: o'_j and s'_j inside their pass, s between
// the passes, r and the positive o at the end.
template <int KPT, bool UNIQ>
__global__ void __launch_bounds__(KT)
k_kge_step_sides_fused(float* __restrict__ slab, const int64_t* __restrict__ keys_s,
                       const int64_t* __restrict__ keys_r, const int64_t* __restrict__ keys_o,
                       const int64_t* __restrict__ keys_neg_o,
                       const int64_t* __restrict__ keys_neg_s, float* __restrict__ loss, int B,
                       int N, int NS, int D, int32_t plen, int world, float lr, float eps,
                       float gamma_e, float gamma_r, const uint32_t* __restrict__ bits,
                       unsigned long long* __restrict__ shared_stat) {
  __shared__ float lds[KT / 64];
  const int dc = D >> 1;
  const int w = UNIQ ? 1 : world;  // as in k_kge_step_fused
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t key_s = keys_s[b], key_r = keys_r[b], key_o = keys_o[b];
    float* sb = row_at(slab, key_s, plen, w);
    float* rb = row_at(slab, key_r, plen, w);
    float* pb = row_at(slab, key_o, plen, w);
    const bool s_shared = row_shared<UNIQ>(bits, key_s);
    const bool r_shared = row_shared<UNIQ>(bits, key_r);
    const bool p_shared = row_shared<UNIQ>(bits, key_o);
    unsigned n_shared = (unsigned)s_shared + (unsigned)r_shared + (unsigned)p_shared;

    float r_re[KPT], r_im[KPT], a_rre[KPT], a_rim[KPT];
    float u_re[KPT], u_im[KPT];
    float lsum = 0.f;
    float c0 = 0.f;
    {
      float s_re[KPT], s_im[KPT], a_sre[KPT], a_sim[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        a_sre[i] = a_sim[i] = a_rre[i] = a_rim[i] = 0.f;
        if (k < dc) {
          s_re[i] = sb[k];
          s_im[i] = sb[dc + k];
          r_re[i] = rb[k];
          r_im[i] = rb[dc + k];
          u_re[i] = s_re[i] * r_re[i] - s_im[i] * r_im[i];
          u_im[i] = s_im[i] * r_re[i] + s_re[i] * r_im[i];
        } else {
          s_re[i] = s_im[i] = r_re[i] = r_im[i] = u_re[i] = u_im[i] = 0.f;
        }
      }

      for (int j = 0; j <= N; ++j) {
        const bool pos = j == 0;
        const int64_t ok = pos ? key_o : keys_neg_o[(int64_t)b * N + (j - 1)];
        float* ob = row_at(slab, ok, plen, w);
        const bool o_shared = pos ? p_shared : row_shared<UNIQ>(bits, ok);
        if (!pos) n_shared += (unsigned)o_shared;
        float y = pos ? 1.f : -1.f;
        float part = 0.f;
        float o_re[KPT], o_im[KPT], Go_re[KPT], Go_im[KPT];
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
          int k = threadIdx.x + i * KT;
          o_re[i] = k < dc ? ob[k] : 0.f;
          o_im[i] = k < dc ? ob[dc + k] : 0.f;
          Go_re[i] = (k < dc && !pos) ? ob[D + k] : 0.f;
          Go_im[i] = (k < dc && !pos) ? ob[D + dc + k] : 0.f;
          part += u_re[i] * o_re[i] + u_im[i] * o_im[i];
        }
        float psi = block_reduce_sum(part, lds);
        float c = -y * sigmoidf(-y * psi);
        if (threadIdx.x == 0) lsum += softplus1pf(-y * psi);
        if (pos) c0 = c;

#pragma unroll
        for (int i = 0; i < KPT; ++i) {
          int k = threadIdx.x + i * KT;
          if (k >= dc) continue;
          a_sre[i] += c * (r_re[i] * o_re[i] + r_im[i] * o_im[i]);
          a_sim[i] += c * (r_re[i] * o_im[i] - r_im[i] * o_re[i]);
          a_rre[i] += c * (s_re[i] * o_re[i] + s_im[i] * o_im[i]);
          a_rim[i] += c * (s_re[i] * o_im[i] - s_im[i] * o_re[i]);
          if (pos) continue;  // the positive object waits for the subject pass
          slab_adagrad_complex(ob, k, dc, D, c * u_re[i], c * u_im[i], o_re[i], o_im[i],
                               Go_re[i], Go_im[i], lr, eps, o_shared);
        }
      }

#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        slab_adagrad_complex(sb, k, dc, D, a_sre[i] + gamma_e * s_re[i],
                             a_sim[i] + gamma_e * s_im[i], s_re[i], s_im[i], sb[D + k],
                             sb[D + dc + k], lr, eps, s_shared);
      }
    }

    float p_re[KPT], p_im[KPT], a_ore[KPT], a_oim[KPT];
    float v_re[KPT], v_im[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      p_re[i] = k < dc ? pb[k] : 0.f;
      p_im[i] = k < dc ? pb[dc + k] : 0.f;
      a_ore[i] = c0 * u_re[i];
      a_oim[i] = c0 * u_im[i];
      v_re[i] = r_re[i] * p_re[i] + r_im[i] * p_im[i];
      v_im[i] = r_re[i] * p_im[i] - r_im[i] * p_re[i];
    }
    for (int j = 0; j < NS; ++j) {
      const int64_t xk = keys_neg_s[(int64_t)b * NS + j];
      float* xb = row_at(slab, xk, plen, w);
      const bool x_shared = row_shared<UNIQ>(bits, xk);
      n_shared += (unsigned)x_shared;
      float part = 0.f;
      float x_re[KPT], x_im[KPT], Gx_re[KPT], Gx_im[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        x_re[i] = k < dc ? xb[k] : 0.f;
        x_im[i] = k < dc ? xb[dc + k] : 0.f;
        Gx_re[i] = k < dc ? xb[D + k] : 0.f;
        Gx_im[i] = k < dc ? xb[D + dc + k] : 0.f;
        part += v_re[i] * x_re[i] + v_im[i] * x_im[i];
      }
      float psi = block_reduce_sum(part, lds);
      float c = sigmoidf(psi);
      if (threadIdx.x == 0) lsum += softplus1pf(psi);
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        if (k >= dc) continue;
        a_rre[i] += c * (x_re[i] * p_re[i] + x_im[i] * p_im[i]);
        a_rim[i] += c * (x_re[i] * p_im[i] - x_im[i] * p_re[i]);
        a_ore[i] += c * (x_re[i] * r_re[i] - x_im[i] * r_im[i]);
        a_oim[i] += c * (x_im[i] * r_re[i] + x_re[i] * r_im[i]);
        slab_adagrad_complex(xb, k, dc, D, c * v_re[i], c * v_im[i], x_re[i], x_im[i], Gx_re[i],
                             Gx_im[i], lr, eps, x_shared);
      }
    }

#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= dc) continue;
      slab_adagrad_complex(rb, k, dc, D, a_rre[i] + gamma_r * r_re[i],
                           a_rim[i] + gamma_r * r_im[i], r_re[i], r_im[i], rb[D + k],
                           rb[D + dc + k], lr, eps, r_shared);
      slab_adagrad_complex(pb, k, dc, D, a_ore[i] + gamma_e * p_re[i],
                           a_oim[i] + gamma_e * p_im[i], p_re[i], p_im[i], pb[D + k],
                           pb[D + dc + k], lr, eps, p_shared);
    }
    if (threadIdx.x == 0) {
      loss[b] = lsum;
      if (UNIQ && shared_stat) atomicAdd(shared_stat, (unsigned long long)n_shared);
    }
  }
}

void kge_complex_step_sides_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                      const int64_t* keys_o, const int64_t* keys_neg_o,
                                      const int64_t* keys_neg_s, float* loss, int B, int N,
                                      int NS, int D, int32_t plen, int world, float lr,
                                      float eps, float gamma_e, float gamma_r, void* stream,
                                      const uint32_t* bits, unsigned long long* shared_stat) {
  if (B < 1) return;
  // the one-sided step is run by its own kernel: see kge_complex_step_sides_gpu
  if (NS == 0 && gamma_e == 0.f && gamma_r == 0.f)
    return kge_complex_step_fused_gpu(slab, keys_s, keys_r, keys_o, keys_neg_o, loss, B, N, D,
                                      plen, world, lr, eps, stream, bits, shared_stat);
  const bool uniq = bits != nullptr && world == 1;  // as in kge_complex_step_fused_gpu
  if (!uniq) bits = nullptr, shared_stat = nullptr;
  dispatch_kpt(D >> 1, [&](auto kpt) {
    constexpr int KPT = decltype(kpt)::value;
    hipLaunchKernelGGL(
        (uniq ? k_kge_step_sides_fused<KPT, true> : k_kge_step_sides_fused<KPT, false>),
        dim3(grid_for(B)), dim3(KT), 0, (hipStream_t)stream, slab, keys_s, keys_r, keys_o,
        keys_neg_o, keys_neg_s, loss, B, N, NS, D, plen, world, lr, eps, gamma_e, gamma_r, bits,
        shared_stat);
  });
}

}  // namespace adapm

namespace adapm {

// Fused SGNS: mirror of k_w2v_step reading rows straight from the slab
// at identity offsets and atomically applying the AdaGrad updates.
template <int KPT>
__global__ void k_w2v_step_fused(float* __restrict__ slab, const int64_t* __restrict__ keys_ctr,
                                 const int64_t* __restrict__ keys_ctx,
                                 const int64_t* __restrict__ keys_neg, float* __restrict__ loss,
                                 int B, int N, int D, int32_t plen, int world, float lr,
                                 float eps) {
  __shared__ float lds[KT / 64];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    float* cb = row_at(slab, keys_ctr[b], plen, world);
    float c_emb[KPT], a_c[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      c_emb[i] = k < D ? cb[k] : 0.f;
      a_c[i] = 0.f;
    }
    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      int64_t xk = (j == 0) ? keys_ctx[b] : keys_neg[(int64_t)b * N + (j - 1)];
      float* xb = row_at(slab, xk, plen, world);
      float y = (j == 0) ? 1.f : -1.f;
      float part = 0.f;
      float x_emb[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        x_emb[i] = k < D ? xb[k] : 0.f;
        part += c_emb[i] * x_emb[i];
      }
      float dot = block_reduce_sum(part, lds);
      float g = -y * sigmoidf(-y * dot);
      if (threadIdx.x == 0) lsum += softplusf(-y * dot);
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        int k = threadIdx.x + i * KT;
        if (k >= D) continue;
        a_c[i] += g * x_emb[i];
        slab_adagrad(&xb[k], &xb[D + k], g * c_emb[i], x_emb[i], xb[D + k], lr, eps,
                     /*shared=*/true);
      }
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= D) continue;
      slab_adagrad(&cb[k], &cb[D + k], a_c[i], c_emb[i], cb[D + k], lr, eps, /*shared=*/true);
    }
    if (threadIdx.x == 0) loss[b] = lsum;
  }
}

// Fused MF: w/h row values are read into registers before any atomic
// write in the same lane, so the NZSL+L2 gradients use a consistent
// pre-update snapshot per nonzero (duplicates across the batch hogwild).
__global__ void k_mf_step_fused(float* __restrict__ slab, const int64_t* __restrict__ keys_w,
                                const int64_t* __restrict__ keys_h, const float* __restrict__ x,
                                float* __restrict__ loss, int B, int R, int32_t plen, int world,
                                float lr, float lambda, float eps) {
  __shared__ float lds[KT / 64];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    float* wb = row_at(slab, keys_w[b], plen, world);
    float* hb = row_at(slab, keys_h[b], plen, world);
    float part = 0.f;
    for (int k = threadIdx.x; k < R; k += KT) part += wb[k] * hb[k];
    float pred = block_reduce_sum(part, lds);
    float e = x[b] - pred;
    if (threadIdx.x == 0) loss[b] = e * e;
    for (int k = threadIdx.x; k < R; k += KT) {
      float wv = wb[k], hv = hb[k];
      float gw = -2.f * e * hv + 2.f * lambda * wv;
      float gh = -2.f * e * wv + 2.f * lambda * hv;
      float Gw = wb[R + k], Gh = hb[R + k];
      slab_adagrad(&wb[k], &wb[R + k], gw, wv, Gw, lr, eps, /*shared=*/true);
      slab_adagrad(&hb[k], &hb[R + k], gh, hv, Gh, lr, eps, /*shared=*/true);
    }
  }
}

void w2v_sgns_step_fused_gpu(float* slab, const int64_t* keys_ctr, const int64_t* keys_ctx,
                             const int64_t* keys_neg, float* loss, int B, int N, int D,
                             int32_t plen, int world, float lr, float eps, void* stream) {
  dispatch_kpt(D, [&](auto kpt) {
    hipLaunchKernelGGL(k_w2v_step_fused<decltype(kpt)::value>, dim3(grid_for(B)), dim3(KT), 0,
                       (hipStream_t)stream, slab, keys_ctr, keys_ctx, keys_neg, loss, B, N, D,
                       plen, world, lr, eps);
  });
}

void mf_update_step_fused_gpu(float* slab, const int64_t* keys_w, const int64_t* keys_h,
                              const float* x, float* loss, int B, int R, int32_t plen,
                              int world, float lr, float lambda, float eps, void* stream) {
  hipLaunchKernelGGL(k_mf_step_fused, dim3(grid_for(B)), dim3(KT), 0, (hipStream_t)stream, slab,
                     keys_w, keys_h, x, loss, B, R, plen, world, lr, lambda, eps);
}

}  // namespace adapm
