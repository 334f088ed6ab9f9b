// CPU backend of the app kernels (kernels.h) — identical math to
// kernels_hip.hip, used by the no-GPU test tier and as the reference for
// GPU numerics tests (alongside plain-torch fp32 references in tests/).
#include <algorithm>
#include <cmath>
#include <vector>

#include "kernels.h"
#include "ustream.h"

namespace adapm {

static inline float sigmoidf_(float x) { return 1.f / (1.f + std::exp(-x)); }
static inline float softplusf_(float x) { return x > 20.f ? x : std::log1p(std::exp(x)); }

void kge_complex_step_cpu(const float* s, const float* r, const float* o, const float* neg,
                          float* ds, float* dr, float* do_, float* dneg, float* loss, int B,
                          int N, int D, float lr, float eps) {
  const int dc = D >> 1;
  const int row = D << 1;
  std::vector<float> a_sre(dc), a_sim(dc), a_rre(dc), a_rim(dc), u_re(dc), u_im(dc);
  for (int b = 0; b < B; ++b) {
    const float* sb = s + (int64_t)b * row;
    const float* rb = r + (int64_t)b * row;
    for (int k = 0; k < dc; ++k) {
      u_re[k] = sb[k] * rb[k] - sb[dc + k] * rb[dc + k];
      u_im[k] = sb[dc + k] * rb[k] + sb[k] * rb[dc + k];
      a_sre[k] = a_sim[k] = a_rre[k] = a_rim[k] = 0.f;
    }
    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      const float* ob = (j == 0) ? o + (int64_t)b * row : neg + ((int64_t)b * N + (j - 1)) * row;
      float* dob = (j == 0) ? do_ + (int64_t)b * row : dneg + ((int64_t)b * N + (j - 1)) * row;
      float y = (j == 0) ? 1.f : -1.f;
      double psi = 0.0;
      for (int k = 0; k < dc; ++k) psi += u_re[k] * ob[k] + u_im[k] * ob[dc + k];
      float c = -y * sigmoidf_(-y * (float)psi);
      lsum += softplusf_(-y * (float)psi);
      for (int k = 0; k < dc; ++k) {
        float o_re = ob[k], o_im = ob[dc + k];
        a_sre[k] += c * (rb[k] * o_re + rb[dc + k] * o_im);
        a_sim[k] += c * (rb[k] * o_im - rb[dc + k] * o_re);
        a_rre[k] += c * (sb[k] * o_re + sb[dc + k] * o_im);
        a_rim[k] += c * (sb[k] * o_im - sb[dc + k] * o_re);
        float g_re = c * u_re[k], g_im = c * u_im[k];
        dob[k] = -lr * g_re / std::sqrt(ob[D + k] + g_re * g_re + eps);
        dob[dc + k] = -lr * g_im / std::sqrt(ob[D + dc + k] + g_im * g_im + eps);
        dob[D + k] = g_re * g_re;
        dob[D + dc + k] = g_im * g_im;
      }
    }
    float* dsb = ds + (int64_t)b * row;
    float* drb = dr + (int64_t)b * row;
    for (int k = 0; k < dc; ++k) {
      dsb[k] = -lr * a_sre[k] / std::sqrt(sb[D + k] + a_sre[k] * a_sre[k] + eps);
      dsb[dc + k] = -lr * a_sim[k] / std::sqrt(sb[D + dc + k] + a_sim[k] * a_sim[k] + eps);
      dsb[D + k] = a_sre[k] * a_sre[k];
      dsb[D + dc + k] = a_sim[k] * a_sim[k];
      drb[k] = -lr * a_rre[k] / std::sqrt(rb[D + k] + a_rre[k] * a_rre[k] + eps);
      drb[dc + k] = -lr * a_rim[k] / std::sqrt(rb[D + dc + k] + a_rim[k] * a_rim[k] + eps);
      drb[D + k] = a_rre[k] * a_rre[k];
      drb[D + dc + k] = a_rim[k] * a_rim[k];
    }
    loss[b] = lsum;
  }
}

// push-ready [delta | g^2] of one lane
static inline void write_delta_(float* d_emb, float* d_acc, float g, float acc, float lr,
                                float eps) {
  *d_emb = -lr * g / std::sqrt(acc + g * g + eps);
  *d_acc = g * g;
}

// Sides step (kernels.h): the object pass is kge_complex_step_cpu's loop
// without the write of the positive object, the subject pass scores s'_j
// against v = conj(r) * o.
void kge_complex_step_sides_cpu(const float* s, const float* r, const float* o,
                                const float* neg_o, const float* neg_s, float* ds, float* dr,
                                float* do_, float* dneg_o, float* dneg_s, float* loss, int B,
                                int N, int NS, int D, float lr, float eps, float gamma_e,
                                float gamma_r) {
  const int dc = D >> 1;
  const int row = D << 1;
  std::vector<float> a_sre(dc), a_sim(dc), a_rre(dc), a_rim(dc), a_ore(dc), a_oim(dc);
  std::vector<float> u_re(dc), u_im(dc), v_re(dc), v_im(dc);
  for (int b = 0; b < B; ++b) {
    const float* sb = s + (int64_t)b * row;
    const float* rb = r + (int64_t)b * row;
    const float* pb = o + (int64_t)b * row;
    for (int k = 0; k < dc; ++k) {
      u_re[k] = sb[k] * rb[k] - sb[dc + k] * rb[dc + k];
      u_im[k] = sb[dc + k] * rb[k] + sb[k] * rb[dc + k];
      a_sre[k] = a_sim[k] = a_rre[k] = a_rim[k] = 0.f;
    }
    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      const float* ob = (j == 0) ? pb : neg_o + ((int64_t)b * N + (j - 1)) * row;
      float y = (j == 0) ? 1.f : -1.f;
      double psi = 0.0;
      for (int k = 0; k < dc; ++k) psi += u_re[k] * ob[k] + u_im[k] * ob[dc + k];
      float c = -y * sigmoidf_(-y * (float)psi);
      lsum += softplusf_(-y * (float)psi);
      for (int k = 0; k < dc; ++k) {
        float o_re = ob[k], o_im = ob[dc + k];
        a_sre[k] += c * (rb[k] * o_re + rb[dc + k] * o_im);
        a_sim[k] += c * (rb[k] * o_im - rb[dc + k] * o_re);
        a_rre[k] += c * (sb[k] * o_re + sb[dc + k] * o_im);
        a_rim[k] += c * (sb[k] * o_im - sb[dc + k] * o_re);
        float g_re = c * u_re[k], g_im = c * u_im[k];
        if (j == 0) {  // the positive object waits for the subject pass
          a_ore[k] = g_re;
          a_oim[k] = g_im;
          continue;
        }
        float* dob = dneg_o + ((int64_t)b * N + (j - 1)) * row;
        write_delta_(&dob[k], &dob[D + k], g_re, ob[D + k], lr, eps);
        write_delta_(&dob[dc + k], &dob[D + dc + k], g_im, ob[D + dc + k], lr, eps);
      }
    }
    for (int k = 0; k < dc; ++k) {
      v_re[k] = rb[k] * pb[k] + rb[dc + k] * pb[dc + k];
      v_im[k] = rb[k] * pb[dc + k] - rb[dc + k] * pb[k];
    }
    for (int j = 0; j < NS; ++j) {
      const float* xb = neg_s + ((int64_t)b * NS + j) * row;
      float* dxb = dneg_s + ((int64_t)b * NS + j) * row;
      double psi = 0.0;
      for (int k = 0; k < dc; ++k) psi += v_re[k] * xb[k] + v_im[k] * xb[dc + k];
      float c = sigmoidf_((float)psi);
      lsum += softplusf_((float)psi);
      for (int k = 0; k < dc; ++k) {
        float x_re = xb[k], x_im = xb[dc + k];
        a_rre[k] += c * (x_re * pb[k] + x_im * pb[dc + k]);
        a_rim[k] += c * (x_re * pb[dc + k] - x_im * pb[k]);
        a_ore[k] += c * (x_re * rb[k] - x_im * rb[dc + k]);
        a_oim[k] += c * (x_im * rb[k] + x_re * rb[dc + k]);
        write_delta_(&dxb[k], &dxb[D + k], c * v_re[k], xb[D + k], lr, eps);
        write_delta_(&dxb[dc + k], &dxb[D + dc + k], c * v_im[k], xb[D + dc + k], lr, eps);
      }
    }
    float* dsb = ds + (int64_t)b * row;
    float* drb = dr + (int64_t)b * row;
    float* dpb = do_ + (int64_t)b * row;
    for (int k = 0; k < dc; ++k) {
      write_delta_(&dsb[k], &dsb[D + k], a_sre[k] + gamma_e * sb[k], sb[D + k], lr, eps);
      write_delta_(&dsb[dc + k], &dsb[D + dc + k], a_sim[k] + gamma_e * sb[dc + k],
                   sb[D + dc + k], lr, eps);
      write_delta_(&drb[k], &drb[D + k], a_rre[k] + gamma_r * rb[k], rb[D + k], lr, eps);
      write_delta_(&drb[dc + k], &drb[D + dc + k], a_rim[k] + gamma_r * rb[dc + k],
                   rb[D + dc + k], lr, eps);
      write_delta_(&dpb[k], &dpb[D + k], a_ore[k] + gamma_e * pb[k], pb[D + k], lr, eps);
      write_delta_(&dpb[dc + k], &dpb[D + dc + k], a_oim[k] + gamma_e * pb[dc + k],
                   pb[D + dc + k], lr, eps);
    }
    loss[b] = lsum;
  }
}

void kge_complex_score_cpu(const float* s, const float* r, const float* cand, float* scores,
                           int B, int E, int D) {
  const int dc = D >> 1;
  const int row = D << 1;
  for (int b = 0; b < B; ++b) {
    const float* sb = s + (int64_t)b * row;
    const float* rb = r + (int64_t)b * row;
    for (int e = 0; e < E; ++e) {
      const float* ob = cand + (int64_t)e * row;
      double psi = 0.0;
      for (int k = 0; k < dc; ++k) {
        float ure = sb[k] * rb[k] - sb[dc + k] * rb[dc + k];
        float uim = sb[dc + k] * rb[k] + sb[k] * rb[dc + k];
        psi += ure * ob[k] + uim * ob[dc + k];
      }
      scores[(int64_t)b * E + e] = (float)psi;
    }
  }
}

// fp32 dot as an fmaf chain in ascending k: the order of the MFMA kernels
static inline float dot_chain_(const float* q, const float* c, int K) {
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = std::fmaf(q[k], c[k], acc);
  return acc;
}

void rank_count_cpu(const float* Q, const float* C, const float* base, int32_t* counts, int B,
                    int E, int K, int qstride, int cstride) {
  for (int b = 0; b < B; ++b) {
    const float* qb = Q + (int64_t)b * qstride;
    int32_t n = 0;
    for (int e = 0; e < E; ++e) {
      float v = dot_chain_(qb, C + (int64_t)e * cstride, K);
      n += (v > base[b] || std::isnan(v)) ? 1 : 0;
    }
    counts[b] += n;
  }
}

void pair_scores_cpu(const float* Q, const float* C, const int32_t* owner, float* out, int P,
                     int K, int qstride, int cstride) {
  for (int p = 0; p < P; ++p)
    out[p] = dot_chain_(Q + (int64_t)owner[p] * qstride, C + (int64_t)p * cstride, K);
}

void w2v_sgns_step_cpu(const float* ctr, const float* ctx, const float* neg, float* dctr,
                       float* dctx, float* dneg, float* loss, int B, int N, int D, float lr,
                       float eps) {
  const int row = D << 1;
  std::vector<float> a_c(D);
  for (int b = 0; b < B; ++b) {
    const float* cb = ctr + (int64_t)b * row;
    std::fill(a_c.begin(), a_c.end(), 0.f);
    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      const float* xb = (j == 0) ? ctx + (int64_t)b * row : neg + ((int64_t)b * N + (j - 1)) * row;
      float* dxb = (j == 0) ? dctx + (int64_t)b * row : dneg + ((int64_t)b * N + (j - 1)) * row;
      float y = (j == 0) ? 1.f : -1.f;
      double dot = 0.0;
      for (int k = 0; k < D; ++k) dot += cb[k] * xb[k];
      float g = -y * sigmoidf_(-y * (float)dot);
      lsum += softplusf_(-y * (float)dot);
      for (int k = 0; k < D; ++k) {
        a_c[k] += g * xb[k];
        float gx = g * cb[k];
        dxb[k] = -lr * gx / std::sqrt(xb[D + k] + gx * gx + eps);
        dxb[D + k] = gx * gx;
      }
    }
    float* dcb = dctr + (int64_t)b * row;
    for (int k = 0; k < D; ++k) {
      dcb[k] = -lr * a_c[k] / std::sqrt(cb[D + k] + a_c[k] * a_c[k] + eps);
      dcb[D + k] = a_c[k] * a_c[k];
    }
    loss[b] = lsum;
  }
}

void mf_update_step_cpu(const float* w, const float* h, const float* x, float* dw, float* dh,
                        float* loss, int B, int R, float lr, float lambda, float eps) {
  const int row = R << 1;
  for (int b = 0; b < B; ++b) {
    const float* wb = w + (int64_t)b * row;
    const float* hb = h + (int64_t)b * row;
    double pred = 0.0;
    for (int k = 0; k < R; ++k) pred += wb[k] * hb[k];
    float e = x[b] - (float)pred;
    loss[b] = e * e;
    float* dwb = dw + (int64_t)b * row;
    float* dhb = dh + (int64_t)b * row;
    for (int k = 0; k < R; ++k) {
      float gw = -2.f * e * hb[k] + 2.f * lambda * wb[k];
      float gh = -2.f * e * wb[k] + 2.f * lambda * hb[k];
      dwb[k] = -lr * gw / std::sqrt(wb[R + k] + gw * gw + eps);
      dwb[R + k] = gw * gw;
      dhb[k] = -lr * gh / std::sqrt(hb[R + k] + gh * gh + eps);
      dhb[R + k] = gh * gh;
    }
  }
}

// In-place AdaGrad of one slab element: emb += delta(g), acc += g^2, with
// the delta taken from the accumulator as it was.
static inline void adagrad_inplace(float& emb, float& acc, float g, float lr, float eps) {
  float G = acc + g * g;
  emb += -lr * g / std::sqrt(G + eps);
  acc += g * g;
}

// Fused slab-direct steps, offsets mode (CPU tier of the world>1 fused
// path: offs_* carry float offsets into the slab, resolved by the host
// metadata pass; math mirrors the GPU fused kernels — object rows are
// updated immediately per negative, s/r accumulated then applied).
void kge_complex_step_fused_offs_cpu(float* slab, const int64_t* offs_s, const int64_t* offs_r,
                                     const int64_t* offs_o, const int64_t* offs_neg, float* loss,
                                     int B, int N, int D, float lr, float eps) {
  const int dc = D >> 1;
  std::vector<float> a_sre(dc), a_sim(dc), a_rre(dc), a_rim(dc), u_re(dc), u_im(dc);
  for (int b = 0; b < B; ++b) {
    float* sb = slab + offs_s[b];
    float* rb = slab + offs_r[b];
    for (int k = 0; k < dc; ++k) {
      u_re[k] = sb[k] * rb[k] - sb[dc + k] * rb[dc + k];
      u_im[k] = sb[dc + k] * rb[k] + sb[k] * rb[dc + k];
      a_sre[k] = a_sim[k] = a_rre[k] = a_rim[k] = 0.f;
    }
    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      float* ob = slab + ((j == 0) ? offs_o[b] : offs_neg[(int64_t)b * N + (j - 1)]);
      float y = (j == 0) ? 1.f : -1.f;
      float psi = 0.f;
      for (int k = 0; k < dc; ++k) psi += u_re[k] * ob[k] + u_im[k] * ob[dc + k];
      float c = -y * sigmoidf_(-y * psi);
      lsum += softplusf_(-y * psi);
      for (int k = 0; k < dc; ++k) {
        float o_re = ob[k], o_im = ob[dc + k];
        a_sre[k] += c * (rb[k] * o_re + rb[dc + k] * o_im);
        a_sim[k] += c * (rb[k] * o_im - rb[dc + k] * o_re);
        a_rre[k] += c * (sb[k] * o_re + sb[dc + k] * o_im);
        a_rim[k] += c * (sb[k] * o_im - sb[dc + k] * o_re);
        adagrad_inplace(ob[k], ob[D + k], c * u_re[k], lr, eps);
        adagrad_inplace(ob[dc + k], ob[D + dc + k], c * u_im[k], lr, eps);
      }
    }
    for (int k = 0; k < dc; ++k) {
      adagrad_inplace(sb[k], sb[D + k], a_sre[k], lr, eps);
      adagrad_inplace(sb[dc + k], sb[D + dc + k], a_sim[k], lr, eps);
      adagrad_inplace(rb[k], rb[D + k], a_rre[k], lr, eps);
      adagrad_inplace(rb[dc + k], rb[D + dc + k], a_rim[k], lr, eps);
    }
    loss[b] = lsum;
  }
}

// Sides step in place, in the order of k_kge_step_sides_fused: s and r are
// read once, o'_j updated as they are scored, s updated between the passes,
// the positive o read again for the subject pass, r and o updated last.
void kge_complex_step_sides_fused_offs_cpu(float* slab, const int64_t* offs_s,
                                           const int64_t* offs_r, const int64_t* offs_o,
                                           const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                           float* loss, int B, int N, int NS, int D, float lr,
                                           float eps, float gamma_e, float gamma_r) {
  const int dc = D >> 1;
  std::vector<float> a_sre(dc), a_sim(dc), a_rre(dc), a_rim(dc), a_ore(dc), a_oim(dc);
  std::vector<float> u_re(dc), u_im(dc), v_re(dc), v_im(dc), sv(D), rv(D), pv(D);
  for (int b = 0; b < B; ++b) {
    float* sb = slab + offs_s[b];
    float* rb = slab + offs_r[b];
    float* pb = slab + offs_o[b];
    std::copy(sb, sb + D, sv.begin());
    std::copy(rb, rb + D, rv.begin());
    for (int k = 0; k < dc; ++k) {
      u_re[k] = sv[k] * rv[k] - sv[dc + k] * rv[dc + k];
      u_im[k] = sv[dc + k] * rv[k] + sv[k] * rv[dc + k];
      a_sre[k] = a_sim[k] = a_rre[k] = a_rim[k] = 0.f;
    }
    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      float* ob = (j == 0) ? pb : slab + offs_neg_o[(int64_t)b * N + (j - 1)];
      float y = (j == 0) ? 1.f : -1.f;
      float psi = 0.f;
      for (int k = 0; k < dc; ++k) psi += u_re[k] * ob[k] + u_im[k] * ob[dc + k];
      float c = -y * sigmoidf_(-y * psi);
      lsum += softplusf_(-y * psi);
      for (int k = 0; k < dc; ++k) {
        float o_re = ob[k], o_im = ob[dc + k];
        a_sre[k] += c * (rv[k] * o_re + rv[dc + k] * o_im);
        a_sim[k] += c * (rv[k] * o_im - rv[dc + k] * o_re);
        a_rre[k] += c * (sv[k] * o_re + sv[dc + k] * o_im);
        a_rim[k] += c * (sv[k] * o_im - sv[dc + k] * o_re);
        if (j == 0) {
          a_ore[k] = c * u_re[k];
          a_oim[k] = c * u_im[k];
          continue;
        }
        adagrad_inplace(ob[k], ob[D + k], c * u_re[k], lr, eps);
        adagrad_inplace(ob[dc + k], ob[D + dc + k], c * u_im[k], lr, eps);
      }
    }
    for (int k = 0; k < dc; ++k) {
      adagrad_inplace(sb[k], sb[D + k], a_sre[k] + gamma_e * sv[k], lr, eps);
      adagrad_inplace(sb[dc + k], sb[D + dc + k], a_sim[k] + gamma_e * sv[dc + k], lr, eps);
    }
    std::copy(pb, pb + D, pv.begin());
    for (int k = 0; k < dc; ++k) {
      v_re[k] = rv[k] * pv[k] + rv[dc + k] * pv[dc + k];
      v_im[k] = rv[k] * pv[dc + k] - rv[dc + k] * pv[k];
    }
    for (int j = 0; j < NS; ++j) {
      float* xb = slab + offs_neg_s[(int64_t)b * NS + j];
      float psi = 0.f;
      for (int k = 0; k < dc; ++k) psi += v_re[k] * xb[k] + v_im[k] * xb[dc + k];
      float c = sigmoidf_(psi);
      lsum += softplusf_(psi);
      for (int k = 0; k < dc; ++k) {
        float x_re = xb[k], x_im = xb[dc + k];
        a_rre[k] += c * (x_re * pv[k] + x_im * pv[dc + k]);
        a_rim[k] += c * (x_re * pv[dc + k] - x_im * pv[k]);
        a_ore[k] += c * (x_re * rv[k] - x_im * rv[dc + k]);
        a_oim[k] += c * (x_im * rv[k] + x_re * rv[dc + k]);
        adagrad_inplace(xb[k], xb[D + k], c * v_re[k], lr, eps);
        adagrad_inplace(xb[dc + k], xb[D + dc + k], c * v_im[k], lr, eps);
      }
    }
    for (int k = 0; k < dc; ++k) {
      adagrad_inplace(rb[k], rb[D + k], a_rre[k] + gamma_r * rv[k], lr, eps);
      adagrad_inplace(rb[dc + k], rb[D + dc + k], a_rim[k] + gamma_r * rv[dc + k], lr, eps);
      adagrad_inplace(pb[k], pb[D + k], a_ore[k] + gamma_e * pv[k], lr, eps);
      adagrad_inplace(pb[dc + k], pb[D + dc + k], a_oim[k] + gamma_e * pv[dc + k], lr, eps);
    }
    loss[b] = lsum;
  }
}

void w2v_sgns_step_fused_offs_cpu(float* slab, const int64_t* offs_ctr, const int64_t* offs_ctx,
                                  const int64_t* offs_neg, float* loss, int B, int N, int D,
                                  float lr, float eps) {
  std::vector<float> a_c(D), c_emb(D);
  for (int b = 0; b < B; ++b) {
    float* cb = slab + offs_ctr[b];
    for (int k = 0; k < D; ++k) {
      c_emb[k] = cb[k];
      a_c[k] = 0.f;
    }
    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      float* xb = slab + ((j == 0) ? offs_ctx[b] : offs_neg[(int64_t)b * N + (j - 1)]);
      float y = (j == 0) ? 1.f : -1.f;
      float dot = 0.f;
      for (int k = 0; k < D; ++k) dot += c_emb[k] * xb[k];
      float g = -y * sigmoidf_(-y * dot);
      lsum += softplusf_(-y * dot);
      for (int k = 0; k < D; ++k) {
        float xv = xb[k];
        a_c[k] += g * xv;
        adagrad_inplace(xb[k], xb[D + k], g * c_emb[k], lr, eps);
      }
    }
    for (int k = 0; k < D; ++k) {
      adagrad_inplace(cb[k], cb[D + k], a_c[k], lr, eps);
    }
    loss[b] = lsum;
  }
}

void mf_update_step_fused_offs_cpu(float* slab, const int64_t* offs_w, const int64_t* offs_h,
                                   const float* x, float* loss, int B, int R, float lr,
                                   float lambda, float eps) {
  for (int b = 0; b < B; ++b) {
    float* wb = slab + offs_w[b];
    float* hb = slab + offs_h[b];
    float pred = 0.f;
    for (int k = 0; k < R; ++k) pred += wb[k] * hb[k];
    float e = x[b] - pred;
    loss[b] = e * e;
    for (int k = 0; k < R; ++k) {
      float wv = wb[k], hv = hb[k];
      float gw = -2.f * e * hv + 2.f * lambda * wv;
      float gh = -2.f * e * wv + 2.f * lambda * hv;
      adagrad_inplace(wb[k], wb[R + k], gw, lr, eps);
      adagrad_inplace(hb[k], hb[R + k], gh, lr, eps);
    }
  }
}

void mf_loss_cpu(const float* w, const float* h, const float* x, float* out2, int B, int R,
                 float lambda) {
  const int row = R << 1;
  double se = 0, reg = 0;
  for (int b = 0; b < B; ++b) {
    const float* wb = w + (int64_t)b * row;
    const float* hb = h + (int64_t)b * row;
    double pred = 0, nrm = 0;
    for (int k = 0; k < R; ++k) {
      pred += wb[k] * hb[k];
      nrm += wb[k] * wb[k] + hb[k] * hb[k];
    }
    double e = x[b] - pred;
    se += e * e;
    reg += lambda * nrm;
  }
  out2[0] += (float)se;
  out2[1] += (float)reg;
}

static inline uint64_t pcg_hash64_c(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

void alias_draw_cpu(const float* prob, const int32_t* alias, int64_t n, uint64_t seed,
                    int64_t N, int64_t* out) {
  for (int64_t i = 0; i < N; ++i) {
    uint64_t h = pcg_hash64_c(seed ^ (uint64_t)i * 0x9e3779b97f4a7c15ULL);
    int64_t slot = (int64_t)(h % (uint64_t)n);
    float u = (float)((h >> 40) & 0xffffff) * (1.0f / 16777216.0f);
    out[i] = (u < prob[slot]) ? slot : (int64_t)alias[slot];
  }
}

// CPU twin of uniform_draw_gpu: the same per-chunk jump-ahead, the same
// scratch (keys in word order here, thread-interleaved on the device), and
// a compaction over the per-block counts.
void uniform_draw_cpu(uint64_t* state, int64_t lo, uint32_t excl, uint32_t thr, int64_t n,
                      int64_t words, int64_t* out, int64_t* tmp) {
  const UStreamRange r{lo, excl, thr};
  const int64_t chunks = ustream_chunks(words), nb = ustream_blocks(words);
  int64_t* counts = tmp + USTREAM_TMP_COUNTS;
  int64_t* keys = counts + nb;
  for (int64_t b = 0; b < nb; ++b) counts[b] = 0;
  for (int64_t c = 0; c < chunks; ++c)
    counts[c / USTREAM_BLOCK] +=
        ustream_gen_chunk(state, r, words, c, keys + c * USTREAM_CHUNK, 1);
  int64_t total = 0, consumed = 0;
  for (int64_t b = 0; b < nb; ++b) {
    int64_t idx = total;  // block offset = sum of the counts before it
    total += counts[b];
    if (idx >= n) continue;
    const int64_t w1 = std::min((b + 1) * (int64_t)USTREAM_BLOCK * USTREAM_CHUNK, words);
    for (int64_t w = b * (int64_t)USTREAM_BLOCK * USTREAM_CHUNK; w < w1 && idx < n; ++w) {
      if (keys[w] == USTREAM_REJECTED) continue;
      out[idx++] = keys[w];
      if (idx == n) consumed = w + 1;
    }
  }
  ustream_finish(state, r, n, words, total, consumed, out);
}

}  // namespace adapm

namespace adapm {

void rescal_step_cpu(const float* s, const float* r, const float* o, const float* neg,
                     float* ds, float* drl, float* do_, float* dneg, float* loss, int B, int N,
                     int D, float lr, float eps) {
  const int erow = 2 * D;
  const int64_t rrow = 2LL * D * D;
  std::vector<float> u(D), w(D), t(D);
  for (int b = 0; b < B; ++b) {
    const float* sb = s + (int64_t)b * erow;
    const float* rb = r + (int64_t)b * rrow;
    // u = R^T e_s
    for (int j = 0; j < D; ++j) {
      double a = 0;
      for (int i = 0; i < D; ++i) a += rb[(int64_t)i * D + j] * sb[i];
      u[j] = (float)a;
    }
    std::fill(w.begin(), w.end(), 0.f);
    float lsum = 0.f;
    for (int j = 0; j <= N; ++j) {
      const float* ob = (j == 0) ? o + (int64_t)b * erow : neg + ((int64_t)b * N + j - 1) * erow;
      float* dob = (j == 0) ? do_ + (int64_t)b * erow : dneg + ((int64_t)b * N + j - 1) * erow;
      float y = (j == 0) ? 1.f : -1.f;
      double dot = 0;
      for (int k = 0; k < D; ++k) dot += u[k] * ob[k];
      float c = -y * sigmoidf_(-y * (float)dot);
      lsum += softplusf_(-y * (float)dot);
      for (int k = 0; k < D; ++k) {
        w[k] += c * ob[k];
        float g = c * u[k];
        dob[k] = -lr * g / std::sqrt(ob[D + k] + g * g + eps);
        dob[D + k] = g * g;
      }
    }
    loss[b] = lsum;
    // de_s = R w
    float* dsb = ds + (int64_t)b * erow;
    for (int i = 0; i < D; ++i) {
      double a = 0;
      for (int k = 0; k < D; ++k) a += rb[(int64_t)i * D + k] * w[k];
      t[i] = (float)a;
      float g = t[i];
      dsb[i] = -lr * g / std::sqrt(sb[D + i] + g * g + eps);
      dsb[D + i] = g * g;
    }
    // dR = e_s w^T
    float* drb = drl + (int64_t)b * rrow;
    for (int i = 0; i < D; ++i) {
      for (int k = 0; k < D; ++k) {
        float g = sb[i] * w[k];
        int64_t idx = (int64_t)i * D + k;
        drb[idx] = -lr * g / std::sqrt(rb[(int64_t)D * D + idx] + g * g + eps);
        drb[(int64_t)D * D + idx] = g * g;
      }
    }
  }
}

// Sides step (kernels.h): rescal_step_cpu's object pass without the write of
// the positive object, then the subject pass against v = R e_o.
void rescal_step_sides_cpu(const float* s, const float* r, const float* o, const float* neg_o,
                           const float* neg_s, float* ds, float* drl, float* do_,
                           float* dneg_o, float* dneg_s, float* loss, int B, int N, int NS,
                           int D, float lr, float eps, float gamma_e, float gamma_r) {
  const int erow = 2 * D;
  const int64_t rrow = 2LL * D * D;
  std::vector<float> u(D), v(D), w(D), z(D);
  for (int b = 0; b < B; ++b) {
    const float* sb = s + (int64_t)b * erow;
    const float* rb = r + (int64_t)b * rrow;
    const float* pb = o + (int64_t)b * erow;
    // u = R^T e_s, v = R e_o
    for (int j = 0; j < D; ++j) {
      double a = 0, c = 0;
      for (int i = 0; i < D; ++i) {
        a += rb[(int64_t)i * D + j] * sb[i];
        c += rb[(int64_t)j * D + i] * pb[i];
      }
      u[j] = (float)a;
      v[j] = (float)c;
    }
    std::fill(w.begin(), w.end(), 0.f);
    std::fill(z.begin(), z.end(), 0.f);
    float lsum = 0.f, c0 = 0.f;
    for (int j = 0; j <= N; ++j) {
      const float* ob = (j == 0) ? pb : neg_o + ((int64_t)b * N + j - 1) * erow;
      float y = (j == 0) ? 1.f : -1.f;
      double dot = 0;
      for (int k = 0; k < D; ++k) dot += u[k] * ob[k];
      float c = -y * sigmoidf_(-y * (float)dot);
      lsum += softplusf_(-y * (float)dot);
      for (int k = 0; k < D; ++k) w[k] += c * ob[k];
      if (j == 0) {  // the positive object waits for the subject pass
        c0 = c;
        continue;
      }
      float* dob = dneg_o + ((int64_t)b * N + j - 1) * erow;
      for (int k = 0; k < D; ++k) write_delta_(&dob[k], &dob[D + k], c * u[k], ob[D + k], lr, eps);
    }
    for (int j = 0; j < NS; ++j) {
      const float* xb = neg_s + ((int64_t)b * NS + j) * erow;
      float* dxb = dneg_s + ((int64_t)b * NS + j) * erow;
      double dot = 0;
      for (int k = 0; k < D; ++k) dot += v[k] * xb[k];
      float a = sigmoidf_((float)dot);
      lsum += softplusf_((float)dot);
      for (int k = 0; k < D; ++k) {
        z[k] += a * xb[k];
        write_delta_(&dxb[k], &dxb[D + k], a * v[k], xb[D + k], lr, eps);
      }
    }
    loss[b] = lsum;
    // de_s = R w + gamma_e e_s, de_o = c0 u + R^T z + gamma_e e_o
    float* dsb = ds + (int64_t)b * erow;
    float* dpb = do_ + (int64_t)b * erow;
    for (int i = 0; i < D; ++i) {
      double a = 0, c = 0;
      for (int k = 0; k < D; ++k) {
        a += rb[(int64_t)i * D + k] * w[k];
        c += rb[(int64_t)k * D + i] * z[k];
      }
      write_delta_(&dsb[i], &dsb[D + i], (float)a + gamma_e * sb[i], sb[D + i], lr, eps);
      write_delta_(&dpb[i], &dpb[D + i], c0 * u[i] + (float)c + gamma_e * pb[i], pb[D + i], lr,
                   eps);
    }
    // dR = e_s w^T + z e_o^T + gamma_r R
    float* drb = drl + (int64_t)b * rrow;
    for (int i = 0; i < D; ++i) {
      for (int k = 0; k < D; ++k) {
        int64_t idx = (int64_t)i * D + k;
        write_delta_(&drb[idx], &drb[(int64_t)D * D + idx],
                     sb[i] * w[k] + z[i] * pb[k] + gamma_r * rb[idx], rb[(int64_t)D * D + idx],
                     lr, eps);
      }
    }
  }
}

}  // namespace adapm
