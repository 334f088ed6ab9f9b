// HIP/gfx950 app kernels — see kernels.h. One workgroup (256 threads =
// 4 waves) per training sample; rows are 2D floats = [emb(D) | accum(D)].
// These kernels are HBM-bound (each pulled row is read once, each delta
// row written once); the arithmetic per element is small, so the design
// goal is coalesced row traffic (one dword per lane, 256 contiguous bytes
// per wave instruction) and cheap block reductions (wave __shfl_xor + one
// LDS hop across the 4 waves).
#include <hip/hip_runtime.h>
#include <algorithm>

#include "kernels.h"
#include "ustream.h"

namespace adapm {

#define KT 256  // threads per workgroup

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
        float g_re = c * u_re[i];
        float g_im = c * u_im[i];
        float G_re = ob[D + k] + g_re * g_re;
        float G_im = ob[D + dc + k] + g_im * g_im;
        dob[k] = -lr * g_re * __frsqrt_rn(G_re + eps);
        dob[dc + k] = -lr * g_im * __frsqrt_rn(G_im + eps);
        dob[D + k] = g_re * g_re;
        dob[D + dc + k] = g_im * g_im;
      }
    }
    // write s/r deltas with fused AdaGrad
    float* dsb = ds + (int64_t)b * row;
    float* drb = dr + (int64_t)b * row;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= dc) continue;
      float Gsr = sb[D + k] + a_sre[i] * a_sre[i];
      float Gsi = sb[D + dc + k] + a_sim[i] * a_sim[i];
      dsb[k] = -lr * a_sre[i] * __frsqrt_rn(Gsr + eps);
      dsb[dc + k] = -lr * a_sim[i] * __frsqrt_rn(Gsi + eps);
      dsb[D + k] = a_sre[i] * a_sre[i];
      dsb[D + dc + k] = a_sim[i] * a_sim[i];
      float Grr = rb[D + k] + a_rre[i] * a_rre[i];
      float Gri = rb[D + dc + k] + a_rim[i] * a_rim[i];
      drb[k] = -lr * a_rre[i] * __frsqrt_rn(Grr + eps);
      drb[dc + k] = -lr * a_rim[i] * __frsqrt_rn(Gri + eps);
      drb[D + k] = a_rre[i] * a_rre[i];
      drb[D + dc + k] = a_rim[i] * a_rim[i];
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
        float gx = g * c_emb[i];
        float G = xb[D + k] + gx * gx;
        dxb[k] = -lr * gx * __frsqrt_rn(G + eps);
        dxb[D + k] = gx * gx;
      }
    }
    float* dcb = dctr + (int64_t)b * row;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= D) continue;
      float G = cb[D + k] + a_c[i] * a_c[i];
      dcb[k] = -lr * a_c[i] * __frsqrt_rn(G + eps);
      dcb[D + k] = a_c[i] * a_c[i];
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
      float Gw = wb[R + k] + gw * gw;
      float Gh = hb[R + k] + gh * gh;
      dwb[k] = -lr * gw * __frsqrt_rn(Gw + eps);
      dwb[R + k] = gw * gw;
      dhb[k] = -lr * gh * __frsqrt_rn(Gh + eps);
      dhb[R + k] = gh * gh;
    }
  }
}

// --------------------------------------------------------------- MF loss

__global__ void k_mf_loss(const float* __restrict__ w, const float* __restrict__ h,
                          const float* __restrict__ x, float* __restrict__ out2, int B, int R,
                          float lambda) {
  __shared__ float lds[2][KT / 64];
  const int row = R << 1;
  float se = 0.f, reg = 0.f;
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
      se += e * e;
      reg += lambda * n2;
    }
  }
  if (threadIdx.x == 0) {
    atomicAdd(&out2[0], se);
    atomicAdd(&out2[1], reg);
  }
}

void mf_loss_gpu(const float* w, const float* h, const float* x, float* out2, int B, int R,
                 float lambda, void* stream) {
  if (B < 1) return;
  int g = B > 16384 ? 16384 : B;
  hipLaunchKernelGGL(k_mf_loss, dim3(g), dim3(KT), 0, (hipStream_t)stream, w, h, x,
                     out2, B, R, lambda);
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

static inline int grid_for(int64_t n) {
  int64_t g = n < 1 ? 1 : n;
  return (int)(g > 16384 ? 16384 : g);
}

void kge_complex_step_gpu(const float* s, const float* r, const float* o, const float* neg,
                          float* ds, float* dr, float* do_, float* dneg, float* loss, int B,
                          int N, int D, float lr, float eps, void* stream) {
  int dc = D >> 1;
  dim3 g(grid_for(B)), t(KT);
  auto st = (hipStream_t)stream;
#define LAUNCH(KPT) \
  hipLaunchKernelGGL(k_kge_step<KPT>, g, t, 0, st, s, r, o, neg, ds, dr, do_, dneg, loss, B, N, \
                     D, lr, eps)
  if (dc <= KT) LAUNCH(1);
  else if (dc <= 2 * KT) LAUNCH(2);
  else if (dc <= 4 * KT) LAUNCH(4);
  else LAUNCH(8);
#undef LAUNCH
}
void kge_complex_score_gpu(const float* s, const float* r, const float* cand, float* scores,
                           int B, int E, int D, void* stream) {
  hipLaunchKernelGGL(k_kge_score, dim3(grid_for((int64_t)B * E)), dim3(KT), 0,
                     (hipStream_t)stream, s, r, cand, scores, B, E, D);
}
void w2v_sgns_step_gpu(const float* ctr, const float* ctx, const float* neg, float* dctr,
                       float* dctx, float* dneg, float* loss, int B, int N, int D, float lr,
                       float eps, void* stream) {
  dim3 g(grid_for(B)), t(KT);
  auto st = (hipStream_t)stream;
#define LAUNCH(KPT) \
  hipLaunchKernelGGL(k_w2v_step<KPT>, g, t, 0, st, ctr, ctx, neg, dctr, dctx, dneg, loss, B, N, \
                     D, lr, eps)
  if (D <= KT) LAUNCH(1);
  else if (D <= 2 * KT) LAUNCH(2);
  else if (D <= 4 * KT) LAUNCH(4);
  else LAUNCH(8);
#undef LAUNCH
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
  int blocks = (int)std::min<int64_t>((N + 255) / 256, 4096);
  hipLaunchKernelGGL(k_alias_draw, dim3(blocks), dim3(256), 0, (hipStream_t)stream, prob, alias,
                     n, seed, N, out);
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
        float g = c * u[k];
        dob[k] = -lr * g * __frsqrt_rn(ob[D + k] + g * g + eps);
        dob[D + k] = g * g;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) loss[b] = lsum;

    // de_s = R w
    float* dsb = ds + (int64_t)b * erow;
    for (int i = threadIdx.x; i < D; i += KT) {
      float a = 0.f;
      for (int k = 0; k < D; ++k) a += Rm[i * D + k] * w[k];
      float g = a;
      dsb[i] = -lr * g * __frsqrt_rn(sb[D + i] + g * g + eps);
      dsb[D + i] = g * g;
    }
    // dR = e_s w^T
    float* drb = drl + (int64_t)b * rrow;
    for (int idx = threadIdx.x; idx < D * D; idx += KT) {
      int i = idx / D, k = idx % D;
      float g = es[i] * w[k];
      drb[idx] = -lr * g * __frsqrt_rn(rb[(int64_t)D * D + idx] + g * g + eps);
      drb[(int64_t)D * D + idx] = g * g;
    }
    __syncthreads();
  }
}

void rescal_step_gpu(const float* s, const float* r, const float* o, const float* neg,
                     float* ds, float* drl, float* do_, float* dneg, float* loss, int B, int N,
                     int D, float lr, float eps, void* stream) {
  size_t smem = (size_t)(D * D + 3 * D + KT / 64) * sizeof(float);
  int blocks = (int)std::min<int64_t>(B, 8192);
  hipLaunchKernelGGL(k_rescal_step, dim3(blocks), dim3(KT), smem, (hipStream_t)stream, s, r, o,
                     neg, ds, drl, do_, dneg, loss, B, N, D, lr, eps);
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

// ---- per-launch row marks (see kernels.h): two bits per slab row, 16
// rows per word. Bit 0 = "an occurrence of this batch names the row",
// bit 1 = "a second one does too".
__device__ inline uint32_t* rowmark_word(uint32_t* marks, int64_t row) { return marks + (row >> 4); }
__device__ inline int rowmark_shift(int64_t row) { return 2 * (int)(row & 15); }

__device__ inline int64_t rowmark_key(const RowMarkKeys& ks, int64_t i) {
  // occurrence i of the concatenated key arrays
  int a = 0;
  while (a < ks.count - 1 && i >= ks.n[a]) {
    i -= ks.n[a];
    ++a;
  }
  return ks.keys[a][i];
}

__global__ void k_rowmark_set(uint32_t* __restrict__ marks, RowMarkKeys ks, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int64_t row = rowmark_key(ks, i);
  uint32_t bit = 1u << rowmark_shift(row);
  uint32_t old = atomicOr(rowmark_word(marks, row), bit);
  if ((old & bit) && !(old & (bit << 1))) atomicOr(rowmark_word(marks, row), bit << 1);
}

// Every word that k_rowmark_set touched held only marks of this batch, so
// storing 0 over it (possibly from several threads) restores all-zero.
__global__ void k_rowmark_clear(uint32_t* __restrict__ marks, RowMarkKeys ks, int64_t total) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  *rowmark_word(marks, rowmark_key(ks, i)) = 0u;
}

void rowmark_set_gpu(uint32_t* marks, const RowMarkKeys& ks, void* stream) {
  int64_t total = 0;
  for (int a = 0; a < ks.count; ++a) total += ks.n[a];
  if (total == 0) return;
  hipLaunchKernelGGL(k_rowmark_set, dim3((unsigned)((total + KT - 1) / KT)), dim3(KT), 0,
                     (hipStream_t)stream, marks, ks, total);
}

void rowmark_clear_gpu(uint32_t* marks, const RowMarkKeys& ks, void* stream) {
  int64_t total = 0;
  for (int a = 0; a < ks.count; ++a) total += ks.n[a];
  if (total == 0) return;
  hipLaunchKernelGGL(k_rowmark_clear, dim3((unsigned)((total + KT - 1) / KT)), dim3(KT), 0,
                     (hipStream_t)stream, marks, ks, total);
}

// UNIQ: is the row shared with another occurrence of this batch? The word
// address depends only on the key, so this load runs beside the row loads
// and is uniform across the block.
template <bool UNIQ>
__device__ inline bool row_shared(const uint32_t* __restrict__ marks, int64_t key) {
  if (!UNIQ) return true;
  return (marks[key >> 4] >> (rowmark_shift(key) + 1)) & 1u;
}

// row = row + delta with a plain store, rounded exactly like the atomic it
// replaces: the add must not be contracted into an fma with the multiply
// that produced delta.
__device__ inline float plain_add(float a, float delta) {
#pragma clang fp contract(off)
  return a + delta;
}

// Fused ComplEx step — see kernels.h. Structure mirrors k_kge_step but
// rows come from / return to the slab itself. UNIQ = false is the
// all-atomic kernel (marks unused); UNIQ = true writes the rows that
// `marks` shows to be unique in this batch with plain stores.
template <int KPT, bool UNIQ>
__global__ void k_kge_step_fused(float* __restrict__ slab, const int64_t* __restrict__ keys_s,
                                 const int64_t* __restrict__ keys_r,
                                 const int64_t* __restrict__ keys_o,
                                 const int64_t* __restrict__ keys_neg, float* __restrict__ loss,
                                 int B, int N, int D, int32_t plen, int world, int rank,
                                 float lr, float eps, const uint32_t* __restrict__ marks,
                                 unsigned long long* __restrict__ shared_stat) {
  __shared__ float lds[KT / 64];
  const int dc = D >> 1;
  // the marks imply the single-rank layout: a constant spares row_at the
  // 64-bit division
  const int w = UNIQ ? 1 : world;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t key_s = keys_s[b], key_r = keys_r[b];
    const float* sb = row_at(slab, key_s, plen, w);
    const float* rb = row_at(slab, key_r, plen, w);
    const bool s_shared = row_shared<UNIQ>(marks, key_s);
    const bool r_shared = row_shared<UNIQ>(marks, key_r);
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
      const bool o_shared = row_shared<UNIQ>(marks, ok);
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
        float G_re = Go_re[i] + g_re * g_re;
        float G_im = Go_im[i] + g_im * g_im;
        float d_re = -lr * g_re * __frsqrt_rn(G_re + eps);
        float d_im = -lr * g_im * __frsqrt_rn(G_im + eps);
        if (o_shared) {
          atomicAdd(&ob[k], d_re);
          atomicAdd(&ob[dc + k], d_im);
          atomicAdd(&ob[D + k], g_re * g_re);
          atomicAdd(&ob[D + dc + k], g_im * g_im);
        } else {
          // only writer of this row in this launch: same sums, plain stores
          ob[k] = plain_add(o_re[i], d_re);
          ob[dc + k] = plain_add(o_im[i], d_im);
          ob[D + k] = plain_add(Go_re[i], g_re * g_re);
          ob[D + dc + k] = plain_add(Go_im[i], g_im * g_im);
        }
      }
    }
    float* dsb = const_cast<float*>(sb);
    float* drb = const_cast<float*>(rb);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= dc) continue;
      float Gs_re = sb[D + k], Gs_im = sb[D + dc + k];
      float Gsr = Gs_re + a_sre[i] * a_sre[i];
      float Gsi = Gs_im + a_sim[i] * a_sim[i];
      float ds_re = -lr * a_sre[i] * __frsqrt_rn(Gsr + eps);
      float ds_im = -lr * a_sim[i] * __frsqrt_rn(Gsi + eps);
      if (s_shared) {
        atomicAdd(&dsb[k], ds_re);
        atomicAdd(&dsb[dc + k], ds_im);
        atomicAdd(&dsb[D + k], a_sre[i] * a_sre[i]);
        atomicAdd(&dsb[D + dc + k], a_sim[i] * a_sim[i]);
      } else {
        dsb[k] = plain_add(s_re[i], ds_re);
        dsb[dc + k] = plain_add(s_im[i], ds_im);
        dsb[D + k] = plain_add(Gs_re, a_sre[i] * a_sre[i]);
        dsb[D + dc + k] = plain_add(Gs_im, a_sim[i] * a_sim[i]);
      }
      float Gr_re = rb[D + k], Gr_im = rb[D + dc + k];
      float Grr = Gr_re + a_rre[i] * a_rre[i];
      float Gri = Gr_im + a_rim[i] * a_rim[i];
      float dr_re = -lr * a_rre[i] * __frsqrt_rn(Grr + eps);
      float dr_im = -lr * a_rim[i] * __frsqrt_rn(Gri + eps);
      if (r_shared) {
        atomicAdd(&drb[k], dr_re);
        atomicAdd(&drb[dc + k], dr_im);
        atomicAdd(&drb[D + k], a_rre[i] * a_rre[i]);
        atomicAdd(&drb[D + dc + k], a_rim[i] * a_rim[i]);
      } else {
        drb[k] = plain_add(r_re[i], dr_re);
        drb[dc + k] = plain_add(r_im[i], dr_im);
        drb[D + k] = plain_add(Gr_re, a_rre[i] * a_rre[i]);
        drb[D + dc + k] = plain_add(Gr_im, a_rim[i] * a_rim[i]);
      }
    }
    if (threadIdx.x == 0) {
      loss[b] = lsum;
      if (UNIQ && shared_stat) atomicAdd(shared_stat, (unsigned long long)n_shared);
    }
  }
}

void kge_complex_step_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                const int64_t* keys_o, const int64_t* keys_neg, float* loss,
                                int B, int N, int D, int32_t plen, int world, int rank,
                                float lr, float eps, void* stream, const uint32_t* marks,
                                unsigned long long* shared_stat) {
  int dc = D >> 1;
  dim3 g((unsigned)std::min<int64_t>(B, 16384)), t(KT);
  auto st = (hipStream_t)stream;
  // marks are indexed by key, which is the row only in the single-rank
  // identity layout; every other addressing mode stays all-atomic
  const bool uniq = marks != nullptr && world == 1;
#define LAUNCHF(KPT)                                                                        \
  do {                                                                                      \
    if (uniq)                                                                               \
      hipLaunchKernelGGL((k_kge_step_fused<KPT, true>), g, t, 0, st, slab, keys_s, keys_r,  \
                         keys_o, keys_neg, loss, B, N, D, plen, world, rank, lr, eps, marks, \
                         shared_stat);                                                      \
    else                                                                                    \
      hipLaunchKernelGGL((k_kge_step_fused<KPT, false>), g, t, 0, st, slab, keys_s, keys_r, \
                         keys_o, keys_neg, loss, B, N, D, plen, world, rank, lr, eps,       \
                         (const uint32_t*)nullptr, (unsigned long long*)nullptr);           \
  } while (0)
  if (dc <= KT) LAUNCHF(1);
  else if (dc <= 2 * KT) LAUNCHF(2);
  else if (dc <= 4 * KT) LAUNCHF(4);
  else LAUNCHF(8);
#undef LAUNCHF
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
        float gx = g * c_emb[i];
        float G = xb[D + k] + gx * gx;
        atomicAdd(&xb[k], -lr * gx * __frsqrt_rn(G + eps));
        atomicAdd(&xb[D + k], gx * gx);
      }
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int k = threadIdx.x + i * KT;
      if (k >= D) continue;
      float G = cb[D + k] + a_c[i] * a_c[i];
      atomicAdd(&cb[k], -lr * a_c[i] * __frsqrt_rn(G + eps));
      atomicAdd(&cb[D + k], a_c[i] * a_c[i]);
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
      float Gw = wb[R + k] + gw * gw;
      float Gh = hb[R + k] + gh * gh;
      atomicAdd(&wb[k], -lr * gw * __frsqrt_rn(Gw + eps));
      atomicAdd(&wb[R + k], gw * gw);
      atomicAdd(&hb[k], -lr * gh * __frsqrt_rn(Gh + eps));
      atomicAdd(&hb[R + k], gh * gh);
    }
  }
}

void w2v_sgns_step_fused_gpu(float* slab, const int64_t* keys_ctr, const int64_t* keys_ctx,
                             const int64_t* keys_neg, float* loss, int B, int N, int D,
                             int32_t plen, int world, float lr, float eps, void* stream) {
  dim3 g((unsigned)std::min<int64_t>(B < 1 ? 1 : B, 16384)), t(KT);
  auto st = (hipStream_t)stream;
#define LAUNCHW(KPT) \
  hipLaunchKernelGGL(k_w2v_step_fused<KPT>, g, t, 0, st, slab, keys_ctr, keys_ctx, keys_neg, \
                     loss, B, N, D, plen, world, lr, eps)
  if (D <= KT) LAUNCHW(1);
  else if (D <= 2 * KT) LAUNCHW(2);
  else if (D <= 4 * KT) LAUNCHW(4);
  else LAUNCHW(8);
#undef LAUNCHW
}

void mf_update_step_fused_gpu(float* slab, const int64_t* keys_w, const int64_t* keys_h,
                              const float* x, float* loss, int B, int R, int32_t plen,
                              int world, float lr, float lambda, float eps, void* stream) {
  hipLaunchKernelGGL(k_mf_step_fused, dim3((unsigned)std::min<int64_t>(B < 1 ? 1 : B, 16384)),
                     dim3(KT), 0, (hipStream_t)stream, slab, keys_w, keys_h, x, loss, B, R,
                     plen, world, lr, lambda, eps);
}

}  // namespace adapm
