// RESCAL sides step with dropout (contract: kernels.h, rescal_step_drop_gpu).
//   k_rescal_drop     one workgroup per tile of <= 16 positives of one group:
//                     scores every triple, finishes the entity rows, leaves the
//                     tile's share of dR in scratch[tile][D*D]
//   k_rescal_drop_dr  per group: tile partials in tile order + gamma_r Bg R,
//                     then R's AdaGrad update
// One body each, instantiated for the two ways of reaching rows: pulled buffers
// in and delta buffers out (classic), or slab + offs[i] updated in place (fused).
//
// What was chosen, and why.
//  * R_g sits in LDS for the whole tile, rows padded to DP = ceil4(D) floats so
//    that every row starts on 16 bytes for any D; the pad is zero. Besides R the
//    workgroup keeps nine DP-vectors: the masked subject and object rows of the
//    current triple, double-buffered (x~, y~), the row sums, and one vector of
//    column-sum partials per wave. D = 196 takes 157 KB of the 160.
//  * Lanes -> (i, j). A wave is four groups of 16 lanes. Group r4 of wave w
//    owns the rows i = 16 n + 4 w + r4, n < NR; lane c16 of a group owns the
//    column quads cq = c16 + 16 m, m < NT (columns 4 cq .. 4 cq + 3). So the 16
//    lanes of a group read 256 consecutive bytes of one row of R with one
//    ds_read_b128: no two lanes of a group share a bank, whatever D is. The
//    stride-D pattern the notes record for k_rescal_step_sides (a lane per row)
//    does not occur. Row sums (M⊙R) y~ reduce over the 16 lanes of a group,
//    four xor-shuffles per row; column sums (M⊙R)^T x~ add up in NT float4 per
//    lane over the lane's NR rows and reduce once per triple, two shuffles
//    across the groups and one LDS vector per wave. All sums have a fixed order.
//  * dR lives in registers: acc[NR][NT][4] per lane, NT = ceil(D/64) and NR the
//    template's row count (4 NT, 13 for NT = 4 since D <= 196), guarded by
//    wave-uniform tests on 16 n + 4 w and 64 m. It is stored once per tile.
//  * A quad of R is exactly what one relation hash serves when D % 4 == 0
//    (ALIGNED); its hash argument is linear in (n, m), so one 64-bit multiply
//    per triple and adds give every quad's argument. For other D a padded quad
//    straddles two flat quads and takes two hashes.
//  * The gradient scale g_t is known only after psi_t's block reduction, so a
//    triple has a scoring sweep and an accumulate sweep. The keep bits of the
//    relation mask are KEPT across the reduction, packed four per quad (16 NT^2
//    bits, at most 7 registers), not hashed again: the hash is the most
//    expensive thing per element (64-bit multiplies run at quarter rate).
//  * The accumulate sweep of triple t does NOT ride with the scoring sweep of
//    t + 1: it reads no R, only the registers and x~ (y~ is still in the
//    registers of the scoring sweep), so merging would save no LDS traffic and
//    would cost a second set of y~ and keep-bit registers.
//  * Three barriers per triple: masked rows written -> sums written -> psi.
//    x~, y~ and the slot of the block reduction alternate between two buffers,
//    which is what makes a fourth barrier unnecessary.
//
// adagrad_delta and the softplus of kernels_hip.hip are repeated here rather
// than shared (kernels.h, above rescal_step_fused_gpu, says why).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace adapm {
namespace {

constexpr int DT = 256;  // threads per workgroup (4 waves)
constexpr uint64_t GOLD = 0x9e3779b97f4a7c15ULL;

// One entity role: pulled rows and their deltas (classic) or offsets (fused)
struct Role {
  const float* in;
  float* out;
  const int64_t* offs;
};

struct DropArgs {
  Role s, o, no, ns;
  const float* rm;  // classic: [G][2 D*D]
  float* drl;
  float* slab;  // fused
  const int64_t* offs_rg;
  const int32_t* starts;
  const int32_t* tiles;
  float* scratch;
  float* loss;
  int N, NS, D;
  float lr, eps, gamma_e, gamma_r;
  uint64_t seed;
  uint32_t thr_e, thr_r;
  float sc_e, sc_r;
};

// pcg_hash64 of k_alias_draw, on x = seed ^ idx * GOLD
__device__ inline uint64_t rd_mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

__device__ inline uint32_t rd_field(uint64_t h, int f) {
  return (uint32_t)(h >> (DROP_FIELD_BITS * f)) & (uint32_t)(DROP_ONE - 1);
}

__device__ inline float rd_adagrad_delta(float g, float acc, float lr, float eps) {
  float G = acc + g * g;
  return -lr * g * __frsqrt_rn(G + eps);
}

__device__ inline float rd_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }

// softplus1pf of kernels_hip.hip
__device__ inline float rd_softplus1pf(float x) {
  if (x > 20.f) return x;
  float t = __expf(x);
  return t < 0.01f ? t * (1.f - t * (0.5f - t * (1.f / 3.f))) : __logf(1.f + t);
}

__device__ inline float4 rd_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline void rd_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

template <bool FUSED>
__device__ inline const float* rd_row(const DropArgs& p, const Role& r, int64_t i) {
  return FUSED ? p.slab + r.offs[i] : r.in + i * 2 * p.D;
}

// Component k of row i of a role gets the AdaGrad update of its gradient g.
template <bool FUSED>
__device__ inline void rd_update(const DropArgs& p, const Role& r, int64_t i, int k, float g) {
  const int D = p.D;
  if (FUSED) {
    float* row = p.slab + r.offs[i];
    const float acc = row[D + k];
    atomicAdd(row + k, rd_adagrad_delta(g, acc, p.lr, p.eps));
    atomicAdd(row + D + k, g * g);
  } else {
    const int64_t at = i * 2 * D;
    r.out[at + k] = rd_adagrad_delta(g, r.in[at + D + k], p.lr, p.eps);
    r.out[at + D + k] = g * g;
  }
}

// floats of LDS for dim D
inline size_t drop_lds_bytes(int D) {
  const size_t DP = (D + 3) & ~3;
  return (D * DP + 9 * DP + 8) * sizeof(float);
}

template <int NT, int NR, bool FUSED, bool ALIGNED>
__global__ void __launch_bounds__(DT) k_rescal_drop(DropArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = p.D, DP = (D + 3) & ~3, DQ = DP >> 2;
  float* Rl = smem;          // [D][DP]
  float* xs = Rl + D * DP;   // [2][DP] masked subject-role row
  float* ys = xs + 2 * DP;   // [2][DP] masked object-role row
  float* al = ys + 2 * DP;   // [DP]    row sums
  float* cl = al + DP;       // [4][DP] column-sum partials, one per wave
  float* red = cl + 4 * DP;  // [2][4]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r4 = lane >> 4, c16 = lane & 15;
  const int g = p.tiles[2 * blockIdx.x], m0 = p.tiles[2 * blockIdx.x + 1];
  const int s0 = p.starts[g];
  const int rows = min(16, p.starts[g + 1] - s0 - m0);
  const int N = p.N, NS = p.NS;
  const uint64_t T = 1 + (uint64_t)N + (uint64_t)NS;
  const int64_t dd = (int64_t)D * D;
  const uint64_t Q = (uint64_t)((dd + 3) >> 2);
  const float* Rg = FUSED ? p.slab + p.offs_rg[g] : p.rm + (int64_t)g * 2 * dd;

  if (ALIGNED) {  // DP == D
    for (int q = tid; q < D * DQ; q += DT) rd_st4(Rl + 4 * q, rd_ld4(Rg + 4 * q));
  } else {
    for (int e = tid; e < D * DP; e += DT) {
      const int i = e / DP, j = e - i * DP;
      Rl[e] = j < D ? Rg[i * D + j] : 0.f;
    }
  }

  float acc[NR][NT][4];
#pragma unroll
  for (int n = 0; n < NR; ++n)
#pragma unroll
    for (int m = 0; m < NT; ++m) acc[n][m][0] = acc[n][m][1] = acc[n][m][2] = acc[n][m][3] = 0.f;

  const bool kd = tid < D;  // this thread owns component tid of the entity rows
  const uint64_t seed_r = ~p.seed;
  const uint64_t step_n = (uint64_t)(16 * DQ) * GOLD;  // ALIGNED: 16 rows further
  int par = 0;                                         // buffer of this triple
  for (int bi = 0; bi < rows; ++bi) {
    const int64_t b = s0 + m0 + bi;
    const float sk = kd ? rd_row<FUSED>(p, p.s, b)[tid] : 0.f;
    const float ok = kd ? rd_row<FUSED>(p, p.o, b)[tid] : 0.f;
    float gs = 0.f, go = 0.f, lsum = 0.f;
    for (int t = 0; t < (int)T; ++t, par ^= 1) {
      const uint64_t q = (uint64_t)b * T + (uint64_t)t;
      const bool oneg = t >= 1 && t <= N, sneg = t > N;
      const int64_t jn = oneg ? b * N + (t - 1) : b * NS + (t - N - 1);
      float x = sk, y = ok;
      if (kd && sneg) x = rd_row<FUSED>(p, p.ns, jn)[tid];
      if (kd && oneg) y = rd_row<FUSED>(p, p.no, jn)[tid];
      float ms = 1.f, mo = 1.f;
      if (p.thr_e) {
        const uint64_t h = rd_mix(p.seed ^ (q * (uint64_t)D + (uint64_t)tid) * GOLD);
        ms = rd_field(h, 0) >= p.thr_e ? p.sc_e : 0.f;
        mo = rd_field(h, 1) >= p.thr_e ? p.sc_e : 0.f;
      }
      float* xb = xs + par * DP;
      float* yb = ys + par * DP;
      if (tid < DP) xb[tid] = ms * x, yb[tid] = mo * y;  // the pad: x = y = 0
      __syncthreads();

      // ---- scoring sweep
      float4 ov[NT], cp[NT];
#pragma unroll
      for (int m = 0; m < NT; ++m) {
        const int cq = c16 + 16 * m;
        ov[m] = cp[m] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (64 * m < D && cq < DQ) ov[m] = rd_ld4(yb + 4 * cq);
      }
      constexpr int KW = (NR * NT * 4 + 31) / 32;
      uint32_t keep[KW];
#pragma unroll
      for (int i = 0; i < KW; ++i) keep[i] = 0u;
      // ALIGNED: GOLD times the flat quad index of (row 4 w + r4, quad c16)
      uint64_t hn = (q * Q + (uint64_t)((4 * w + r4) * DQ + c16)) * GOLD;
#pragma unroll
      for (int n = 0; n < NR; ++n) {
        const int rb = 16 * n + 4 * w;  // the same for a whole wave
        if (rb < D) {
          const int i = rb + r4;
          const bool rok = i < D;
          const float xi = rok ? xb[i] : 0.f;
          float rp = 0.f;
#pragma unroll
          for (int m = 0; m < NT; ++m) {
            if (64 * m >= D) continue;
            const int cq = c16 + 16 * m;
            float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rok && cq < DQ) rv = rd_ld4(Rl + i * DP + 4 * cq);
            uint32_t kb = 15u;
            if (p.thr_r) {
              if (ALIGNED) {
                const uint64_t h = rd_mix(seed_r ^ (hn + (uint64_t)(16 * m) * GOLD));
                kb = (uint32_t)(rd_field(h, 0) >= p.thr_r) | (uint32_t)(rd_field(h, 1) >= p.thr_r) << 1 |
                     (uint32_t)(rd_field(h, 2) >= p.thr_r) << 2 | (uint32_t)(rd_field(h, 3) >= p.thr_r) << 3;
              } else {
                // columns 4 cq + c of row i are the flat elements e0 + c
                const uint32_t e0 = (uint32_t)(i * D + 4 * cq);
                const uint64_t fq = q * Q + (uint64_t)(e0 >> 2);
                const uint64_t ha = rd_mix(seed_r ^ fq * GOLD);
                const uint64_t hb = rd_mix(seed_r ^ (fq + 1) * GOLD);
                kb = 0u;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                  const uint32_t sh = (e0 & 3u) + (uint32_t)c;
                  kb |= (uint32_t)(rd_field(sh < 4u ? ha : hb, (int)(sh & 3u)) >= p.thr_r) << c;
                }
              }
            }
            rv.x = (kb & 1u) ? rv.x : 0.f;
            rv.y = (kb & 2u) ? rv.y : 0.f;
            rv.z = (kb & 4u) ? rv.z : 0.f;
            rv.w = (kb & 8u) ? rv.w : 0.f;
            rp += rv.x * ov[m].x + rv.y * ov[m].y + rv.z * ov[m].z + rv.w * ov[m].w;
            cp[m].x += rv.x * xi, cp[m].y += rv.y * xi, cp[m].z += rv.z * xi, cp[m].w += rv.w * xi;
            keep[((n * NT + m) * 4) >> 5] |= kb << (((n * NT + m) * 4) & 31);
          }
          for (int off = 8; off > 0; off >>= 1) rp += __shfl_xor(rp, off, 64);
          if (c16 == 0 && rok) al[i] = rp;
        }
        hn += step_n;
      }
#pragma unroll
      for (int m = 0; m < NT; ++m) {
        if (64 * m >= D) continue;
        const int cq = c16 + 16 * m;
        float4 v = cp[m];
        for (int off = 16; off <= 32; off <<= 1) {
          v.x += __shfl_xor(v.x, off, 64), v.y += __shfl_xor(v.y, off, 64);
          v.z += __shfl_xor(v.z, off, 64), v.w += __shfl_xor(v.w, off, 64);
        }
        if (r4 == 0 && cq < DQ) rd_st4(cl + w * DP + 4 * cq, v);
      }
      __syncthreads();

      // ---- psi, the gradient scale, the entity rows
      float a = 0.f, bs = 0.f;
      if (kd) {
        a = p.sc_r * al[tid];
        bs = p.sc_r * ((cl[tid] + cl[DP + tid]) + (cl[2 * DP + tid] + cl[3 * DP + tid]));
      }
      float part = kd ? xb[tid] * a : 0.f;
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
      float* rs = red + 4 * par;
      if (lane == 0) rs[w] = part;
      __syncthreads();
      const float psi = (rs[0] + rs[1]) + (rs[2] + rs[3]);
      const float yl = t == 0 ? 1.f : -1.f;
      const float c = -yl * rd_sigmoid(-yl * psi);  // dL/dpsi, L = softplus(-y psi)
      lsum += rd_softplus1pf(-yl * psi);
      if (kd) {
        const float gx = c * ms * a, gy = c * mo * bs;
        if (sneg) rd_update<FUSED>(p, p.ns, jn, tid, gx);
        else gs += gx;
        if (oneg) rd_update<FUSED>(p, p.no, jn, tid, gy);
        else go += gy;
      }

      // ---- accumulate sweep: dR += c * M ⊙ (x~ y~^T)
      const float cg = c * p.sc_r;
#pragma unroll
      for (int n = 0; n < NR; ++n) {
        const int rb = 16 * n + 4 * w;
        if (rb >= D) continue;
        const int i = rb + r4;
        const float cx = i < D ? cg * xb[i] : 0.f;
#pragma unroll
        for (int m = 0; m < NT; ++m) {
          if (64 * m >= D) continue;
          const uint32_t kb = keep[((n * NT + m) * 4) >> 5] >> (((n * NT + m) * 4) & 31);
          acc[n][m][0] += (kb & 1u) ? cx * ov[m].x : 0.f;
          acc[n][m][1] += (kb & 2u) ? cx * ov[m].y : 0.f;
          acc[n][m][2] += (kb & 4u) ? cx * ov[m].z : 0.f;
          acc[n][m][3] += (kb & 8u) ? cx * ov[m].w : 0.f;
        }
      }
    }
    if (kd) {
      rd_update<FUSED>(p, p.s, b, tid, gs + p.gamma_e * sk);
      rd_update<FUSED>(p, p.o, b, tid, go + p.gamma_e * ok);
    }
    if (tid == 0) p.loss[b] = lsum;
  }

  float* sc = p.scratch + (int64_t)blockIdx.x * dd;
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    const int i = 16 * n + 4 * w + r4;
    if (i >= D) continue;
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      const int cq = c16 + 16 * m;
      if (64 * m >= D || cq >= DQ) continue;
      if (ALIGNED) {
        rd_st4(sc + (int64_t)i * D + 4 * cq,
               make_float4(acc[n][m][0], acc[n][m][1], acc[n][m][2], acc[n][m][3]));
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (4 * cq + c < D) sc[(int64_t)i * D + 4 * cq + c] = acc[n][m][c];
      }
    }
  }
}

// grid (n_tiles, y): the workgroups of a group's FIRST tile add the group's
// partials, the others have nothing to do.
template <bool FUSED>
__global__ void __launch_bounds__(DT) k_rescal_drop_dr(DropArgs p) {
  const int ti = blockIdx.x;
  if (p.tiles[2 * ti + 1] != 0) return;
  const int g = p.tiles[2 * ti];
  const int Bg = p.starts[g + 1] - p.starts[g];
  const int nt = (Bg + 15) / 16;
  const int64_t dd = (int64_t)p.D * p.D;
  const float* part = p.scratch + (int64_t)ti * dd;
  const float gr = p.gamma_r * (float)Bg;
  for (int64_t e = (int64_t)blockIdx.y * DT + threadIdx.x; e < dd; e += (int64_t)gridDim.y * DT) {
    float sum = part[e];
    for (int k = 1; k < nt; ++k) sum += part[(int64_t)k * dd + e];
    if (FUSED) {
      float* R = p.slab + p.offs_rg[g];
      const float gt = sum + gr * R[e];
      const float a = R[dd + e];
      atomicAdd(R + e, rd_adagrad_delta(gt, a, p.lr, p.eps));
      atomicAdd(R + dd + e, gt * gt);
    } else {
      const float* R = p.rm + (int64_t)g * 2 * dd;
      float* d = p.drl + (int64_t)g * 2 * dd;
      const float gt = sum + gr * R[e];
      d[e] = rd_adagrad_delta(gt, R[dd + e], p.lr, p.eps);
      d[dd + e] = gt * gt;
    }
  }
}

template <int NT, int NR, bool FUSED>
void launch_tiles(const DropArgs& p, int n_tiles, bool aligned, hipStream_t st) {
  const size_t lds = drop_lds_bytes(p.D);
  if (FUSED || aligned)
    hipLaunchKernelGGL((k_rescal_drop<NT, NR, FUSED, true>), dim3(n_tiles), dim3(DT), lds, st, p);
  else
    hipLaunchKernelGGL((k_rescal_drop<NT, NR, false, false>), dim3(n_tiles), dim3(DT), lds, st, p);
}

template <bool FUSED>
void launch_drop(const DropArgs& p, int n_tiles, bool aligned, hipStream_t st) {
  const int D = p.D;
  switch ((D + 63) / 64) {
    case 1: launch_tiles<1, 4, FUSED>(p, n_tiles, aligned, st); break;
    case 2: launch_tiles<2, 8, FUSED>(p, n_tiles, aligned, st); break;
    case 3: launch_tiles<3, 12, FUSED>(p, n_tiles, aligned, st); break;
    default: launch_tiles<4, 13, FUSED>(p, n_tiles, aligned, st); break;  // D <= 196 < 16 * 13
  }
  const int64_t dd = (int64_t)D * D;
  const unsigned gy = (unsigned)std::min<int64_t>((dd + 4 * DT - 1) / (4 * DT), 64);
  hipLaunchKernelGGL(k_rescal_drop_dr<FUSED>, dim3(n_tiles, gy), dim3(DT), 0, st, p);
}
static_assert(RESCAL_DROP_MAX_DIM <= 16 * 13 && RESCAL_DROP_MAX_DIM % 4 == 0, "NT = 4 rows");

inline void drop_fill(DropArgs& p, const int32_t* starts, const int32_t* tiles, float* scratch,
                      float* loss, int N, int NS, int D, float lr, float eps, float gamma_e,
                      float gamma_r, int thr_e, int thr_r, uint64_t seed) {
  p.starts = starts, p.tiles = tiles, p.scratch = scratch, p.loss = loss;
  p.N = N, p.NS = NS, p.D = D;
  p.lr = lr, p.eps = eps, p.gamma_e = gamma_e, p.gamma_r = gamma_r;
  p.seed = seed, p.thr_e = (uint32_t)thr_e, p.thr_r = (uint32_t)thr_r;
  p.sc_e = drop_scale(thr_e), p.sc_r = drop_scale(thr_r);
}

}  // namespace

void rescal_step_drop_gpu(const float* s, const float* rm, const float* o, const float* neg_o,
                          const float* neg_s, float* ds, float* drl, float* do_, float* dneg_o,
                          float* dneg_s, const int32_t* starts, const int32_t* tiles, int n_tiles,
                          float* scratch, float* loss, int B, int G, int N, int NS, int D,
                          float lr, float eps, float gamma_e, float gamma_r, int thr_e, int thr_r,
                          uint64_t drop_seed, void* stream) {
  if (B < 1 || G < 1 || n_tiles < 1) return;
  DropArgs p{};
  p.s = {s, ds, nullptr}, p.o = {o, do_, nullptr};
  p.no = {neg_o, dneg_o, nullptr}, p.ns = {neg_s, dneg_s, nullptr};
  p.rm = rm, p.drl = drl;
  drop_fill(p, starts, tiles, scratch, loss, N, NS, D, lr, eps, gamma_e, gamma_r, thr_e, thr_r,
            drop_seed);
  const bool aligned = D % 4 == 0 && (((uintptr_t)rm | (uintptr_t)scratch) & 15) == 0;
  launch_drop<false>(p, n_tiles, aligned, (hipStream_t)stream);
}

void rescal_step_drop_fused_gpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                                const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                const int64_t* offs_rg, const int32_t* starts,
                                const int32_t* tiles, int n_tiles, float* scratch, float* loss,
                                int B, int G, int N, int NS, int D, float lr, float eps,
                                float gamma_e, float gamma_r, int thr_e, int thr_r,
                                uint64_t drop_seed, void* stream) {
  if (B < 1 || G < 1 || n_tiles < 1) return;
  DropArgs p{};
  p.s = {nullptr, nullptr, offs_s}, p.o = {nullptr, nullptr, offs_o};
  p.no = {nullptr, nullptr, offs_neg_o}, p.ns = {nullptr, nullptr, offs_neg_s};
  p.slab = slab, p.offs_rg = offs_rg;
  drop_fill(p, starts, tiles, scratch, loss, N, NS, D, lr, eps, gamma_e, gamma_r, thr_e, thr_r,
            drop_seed);
  launch_drop<true>(p, n_tiles, true, (hipStream_t)stream);
}

}  // namespace adapm
