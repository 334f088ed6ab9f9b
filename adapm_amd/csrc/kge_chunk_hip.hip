// ComplEx step with chunk-shared negatives (contract: kernels.h,
// kge_complex_step_chunk). With u_b = s_b * r_b laid out as the real vector
// [u_re | u_im] of length D, psi(s_b, r_b, n_j) = u_b . n_j, so one chunk of
// C positives and its M negatives is three small GEMMs on
// v_mfma_f32_16x16x4_f32 (exact f32). Two launches:
//
//   k_chunk_scores  workgroup (chunk, block of 64 negatives): P = U N^T over
//                   K = D; writes G = sigmoid(P) to a scratch [B][M], the
//                   block's share of every loss to lossp[B][4], and (the
//                   workgroup of block 0) psi0 = u_b . o_b as g0[B]
//   k_chunk_update  workgroup (chunk, block of 32 complex columns): A = G N +
//                   g0 o (K = M) and dN = G^T U (K = C) for those columns,
//                   g_s, g_r, g_o from A in registers, then the AdaGrad write
//                   of exactly those columns of every row of the chunk; the
//                   workgroup of column block 0 adds up loss[b]
//
// Both exist for pulled rows (row i of a role at i * 2D, output the push-ready
// [delta | g^2]) and for slab rows (row_at(key), AdaGrad in place, plain
// stores where the row-tag bitmap says the row is unique in the batch). The
// mode only changes how a row is found and how an element is written (RowRef,
// write_elem); the tile bodies are the same.
//
// MFMA lane mapping (wave of 64, x = lane & 15, kk = lane >> 4): the lane
// supplies A[row x][k kk] and B[k kk][col x] and holds, in accumulator
// element r, the output (row 4*kk + r, col x).
//
// k_chunk_scores. A K-chunk is 16 complex columns, i.e. K = 32: the 16 u_re
// and the 16 u_im against n_re and n_im of the same columns, which is why
// D % 8 == 0 is required (float4 loads in either half, no chunk straddling
// re and im). Thread t stages row t >> 2, complex columns 4 * (t & 3): it
// loads s_re, s_im, r_re, r_im as float4, forms u there and stores it, so U
// never exists in memory; the same thread loads n_re, n_im of negative t >> 2.
// The workgroup of block 0 also loads o and keeps its share of u . o, joined
// over the 4 threads of a row by two shuffles. LDS is la[64][36] and
// lb[64][36] twice over (double buffer, one barrier per chunk, 36,864 B):
// rows padded from 32 to 36 floats so that they stay 16-byte aligned and the
// float4 reads of 16 consecutive rows do not all start in one bank group, as
// in rescal_fused_hip.hip. Wave w owns rows 16w.. of the chunk and all four
// 16-column tiles of the block: 4 accumulators, lane k = 8*kk + i for MFMA i
// read as two float4 per operand. Rows past the chunk's end, negatives past M
// and columns past D/2 are staged as zeros; the MFMA loop has no branch.
//
// k_chunk_update. Dynamic LDS, three arrays with rows padded by 4 floats:
//   Ut[64][Cp + 4]   u of the block's columns, transposed: [col][b]
//   Nt[64][Mp + 4]   the negatives' columns, transposed: [col][j]
//   Gl[Cp][Mp + 4]   the chunk's G
// (columns 0..31 the re half, 32..63 the im half; Cp, Mp = C, M rounded up to
// 16, everything outside the chunk zero.) Row strides are 4 mod 16, so the
// operand reads `row x, k kk` (Gl in A = G N, Nt and Ut as B operands) fall in
// 64 different banks; only Gl read as G^T (k along rows) overlaps, 4-way at
// worst, for one of the four operand streams. Staging reads 128 contiguous
// bytes of a row with 8 lanes and stores transposed.
//   A = G N: wave w takes the complex tile w & 1 (16 columns, re and im
//   accumulator) of the positives' tiles w >> 1 and (w >> 1) + 2; it needs
//   both halves to form g_s = a conj(r) and g_r = a conj(s). All gradients of
//   s, r and o are formed, from embeddings read before any write of this
//   workgroup, and held in registers across a barrier; then they are written.
//   dN = G^T U: wave w takes the 16 real columns w of the 64 and walks the
//   negatives' tiles with one accumulator.
// Nothing the workgroup writes is read by it afterwards except the
// accumulator element an AdaGrad write itself belongs to.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
// docs/NOTES_NEXT_ROUND.md has the table; none of the four uses scratch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace adapm {
namespace {

constexpr int CT = 256;        // threads per workgroup (4 waves)
constexpr int KP = 36;         // floats per LDS row of the scores tiles
constexpr int SB = 64;         // negatives per scores workgroup
constexpr int LOSS_PARTS = 4;  // KGE_CHUNK_MAX_M / SB
constexpr int UW = 32;         // complex columns per update workgroup
static_assert(KGE_CHUNK_MAX_C == 64, "a chunk's positives are four 16-row tiles, one per wave");
static_assert(KGE_CHUNK_MAX_M == SB * LOSS_PARTS, "lossp holds one share per block of negatives");
using f32x4 = __attribute__((ext_vector_type(4))) float;

// adagrad_delta, softplus1pf, sigmoidf, plain_add of kernels_hip.hip, repeated
// (kernels.h, above rescal_step_fused_gpu, says why they are not shared)
__device__ inline float kc_adagrad_delta(float g, float acc, float lr, float eps) {
  float G = acc + g * g;
  return -lr * g * __frsqrt_rn(G + eps);
}
__device__ inline float kc_softplus1pf(float x) {
  if (x > 20.f) return x;
  float t = __expf(x);
  return t < 0.01f ? t * (1.f - t * (0.5f - t * (1.f / 3.f))) : __logf(1.f + t);
}
__device__ inline float kc_sigmoidf(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ inline float kc_plain_add(float a, float delta) {
#pragma clang fp contract(off)
  return a + delta;
}

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

enum { ROLE_S = 0, ROLE_R = 1, ROLE_O = 2, ROLE_N = 3 };

struct ChunkArgs {
  // pulled rows: role -> [n][2D] inputs and outputs
  const float* in[4];
  float* out[4];
  // slab rows: role -> device keys
  float* slab;
  const int64_t* keys[4];
  const uint32_t* bits;  // null: every write is atomic
  int32_t plen;
  int world;
  float* G;      // [B][M]
  float* g0;     // [B]
  float* lossp;  // [B][LOSS_PARTS]
  float* loss;   // [B]
  int B, C, M, D;
  float lr, eps;
};

// Where occurrence i of a role is read and written.
struct RowRef {
  const float* in;
  float* out;
  bool shared;
};

template <bool SLAB>
__device__ inline RowRef row_ref(const ChunkArgs& p, int role, int64_t i) {
  RowRef rr;
  if (SLAB) {
    const int64_t key = p.keys[role][i];
    // row_at of kernels_hip.hip
    float* row = p.world ? p.slab + (key / p.world) * (int64_t)p.plen : p.slab + key;
    rr.in = row;
    rr.out = row;
    rr.shared = p.bits ? (p.bits[key >> 5] >> (int)(key & 31)) & 1u : true;
  } else {
    rr.in = p.in[role] + i * 2 * (int64_t)p.D;
    rr.out = p.out[role] + i * 2 * (int64_t)p.D;
    rr.shared = false;
  }
  return rr;
}

// One element's AdaGrad update. Pulled rows: the pair [delta | g^2] as
// write_delta. Slab rows: slab_adagrad of kernels_hip.hip, atomics on a shared
// row, a plain store over the values read here on a row unique in the batch.
template <bool SLAB>
__device__ inline void write_elem(const RowRef& rr, int col, int D, float g, float lr, float eps) {
  const float acc = rr.in[D + col];
  const float d = kc_adagrad_delta(g, acc, lr, eps);
  if (!SLAB) {
    rr.out[col] = d;
    rr.out[D + col] = g * g;
  } else if (rr.shared) {
    atomicAdd(&rr.out[col], d);
    atomicAdd(&rr.out[D + col], g * g);
  } else {
    rr.out[col] = kc_plain_add(rr.in[col], d);
    rr.out[D + col] = kc_plain_add(acc, g * g);
  }
}

struct ScoreLds {
  float a[64][KP];
  float b[SB][KP];
};

template <bool SLAB>
__global__ void __launch_bounds__(CT) k_chunk_scores(ChunkArgs p, int mblocks) {
  __shared__ ScoreLds lds[2];
  __shared__ float l_psi0[64], l_sum[64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int x = lane & 15, kk = lane >> 4;
  const int c = blockIdx.x / mblocks, jb = blockIdx.x % mblocks;
  const int D = p.D, dc = D >> 1, M = p.M;
  const int b0 = c * p.C;
  const int Cc = min(p.C, p.B - b0);
  const int j0 = jb * SB;
  const bool with_o = jb == 0;

  // staging: row `sr` of either tile, complex columns 4 * sq of the chunk
  const int sr = t >> 2, sq = (t & 3) * 4;
  const float *ps = nullptr, *pr = nullptr, *po = nullptr, *pn = nullptr;
  if (sr < Cc) {
    ps = row_ref<SLAB>(p, ROLE_S, b0 + sr).in;
    pr = row_ref<SLAB>(p, ROLE_R, b0 + sr).in;
    if (with_o) po = row_ref<SLAB>(p, ROLE_O, b0 + sr).in;
  }
  if (j0 + sr < M) pn = row_ref<SLAB>(p, ROLE_N, (int64_t)c * M + j0 + sr).in;

  float4 u_re, u_im, n_re, n_im;
  float psi0 = 0.f;
  auto load_chunk = [&](int k0) {  // k0: first complex column
    u_re = u_im = n_re = n_im = zero4();
    const int k = k0 + sq;
    if (k >= dc) return;
    if (ps) {
      const float4 sre = ld4(ps + k), sim = ld4(ps + dc + k);
      const float4 rre = ld4(pr + k), rim = ld4(pr + dc + k);
      u_re = make_float4(sre.x * rre.x - sim.x * rim.x, sre.y * rre.y - sim.y * rim.y,
                         sre.z * rre.z - sim.z * rim.z, sre.w * rre.w - sim.w * rim.w);
      u_im = make_float4(sim.x * rre.x + sre.x * rim.x, sim.y * rre.y + sre.y * rim.y,
                         sim.z * rre.z + sre.z * rim.z, sim.w * rre.w + sre.w * rim.w);
      if (po) {
        const float4 ore = ld4(po + k), oim = ld4(po + dc + k);
        psi0 += u_re.x * ore.x + u_re.y * ore.y + u_re.z * ore.z + u_re.w * ore.w +
                u_im.x * oim.x + u_im.y * oim.y + u_im.z * oim.z + u_im.w * oim.w;
      }
    }
    if (pn) {
      n_re = ld4(pn + k);
      n_im = ld4(pn + dc + k);
    }
  };
  auto store_chunk = [&](ScoreLds& L) {
    *reinterpret_cast<float4*>(&L.a[sr][sq]) = u_re;
    *reinterpret_cast<float4*>(&L.a[sr][16 + sq]) = u_im;
    *reinterpret_cast<float4*>(&L.b[sr][sq]) = n_re;
    *reinterpret_cast<float4*>(&L.b[sr][16 + sq]) = n_im;
  };

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};

  const int nchunks = (dc + 15) / 16;
  load_chunk(0);
  store_chunk(lds[0]);
  __syncthreads();
  for (int ch = 0; ch < nchunks; ++ch) {
    const bool more = ch + 1 < nchunks;
    if (more) load_chunk((ch + 1) * 16);
    const ScoreLds& L = lds[ch & 1];
    const float4 a0 = ld4(&L.a[16 * wave + x][kk * 8]), a1 = ld4(&L.a[16 * wave + x][kk * 8 + 4]);
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 q0 = ld4(&L.b[16 * j + x][kk * 8]), q1 = ld4(&L.b[16 * j + x][kk * 8 + 4]);
      const float bv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc[j], 0, 0, 0);
    }
    if (more) store_chunk(lds[(ch + 1) & 1]);
    __syncthreads();
  }

  // G and the block's share of the loss. Element r of acc[j]: positive
  // 16 * wave + 4 * kk + r, negative j0 + 16 * j + x.
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = j0 + 16 * j + x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wave + 4 * kk + r;
      if (col < M && row < Cc) {
        const float psi = acc[j][r];
        p.G[(int64_t)(b0 + row) * M + col] = kc_sigmoidf(psi);
        rs[r] += kc_softplus1pf(psi);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    for (int off = 8; off > 0; off >>= 1) rs[r] += __shfl_xor(rs[r], off, 64);
    if (x == 0) l_sum[16 * wave + 4 * kk + r] = rs[r];
  }
  if (with_o) {
    psi0 += __shfl_xor(psi0, 1, 64);
    psi0 += __shfl_xor(psi0, 2, 64);
    if ((t & 3) == 0) l_psi0[sr] = psi0;
  }
  __syncthreads();
  if (t < Cc) {
    float part = l_sum[t];
    if (with_o) {
      const float z = l_psi0[t];
      p.g0[b0 + t] = -kc_sigmoidf(-z);
      part += kc_softplus1pf(-z);
    }
    p.lossp[(int64_t)(b0 + t) * LOSS_PARTS + jb] = part;
  }
}

template <bool SLAB>
__global__ void __launch_bounds__(CT) k_chunk_update(ChunkArgs p, int cblocks, int Cp, int Mp) {
  extern __shared__ float smem[];
  const int US = Cp + 4, NS = Mp + 4;
  float* Ut = smem;            // [64][US]
  float* Nt = Ut + 64 * US;    // [64][NS]
  float* Gl = Nt + 64 * NS;    // [Cp][NS]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int x = lane & 15, kk = lane >> 4;
  const int c = blockIdx.x / cblocks, cb = blockIdx.x % cblocks;
  const int D = p.D, dc = D >> 1, M = p.M;
  const int b0 = c * p.C;
  const int Cc = min(p.C, p.B - b0);
  const int k0 = cb * UW;  // first complex column of the block

  // loss[b]: the shares in block order, one workgroup per chunk
  if (cb == 0 && t < Cc) {
    const int parts = (M + SB - 1) / SB;
    float l = 0.f;
    for (int i = 0; i < parts; ++i) l += p.lossp[(int64_t)(b0 + t) * LOSS_PARTS + i];
    p.loss[b0 + t] = l;
  }

  // ---- stage. 8 lanes read 32 consecutive floats of one half of a row.
  const int c4 = (t & 7) * 4;
  const bool col_ok = k0 + c4 < dc;
  {  // Ut: row t >> 3 of 32 per pass, u formed here
    for (int b = t >> 3; b < Cp; b += 32) {
      float4 u_re = zero4(), u_im = zero4();
      if (b < Cc && col_ok) {
        const float* ps = row_ref<SLAB>(p, ROLE_S, b0 + b).in + k0 + c4;
        const float* pr = row_ref<SLAB>(p, ROLE_R, b0 + b).in + k0 + c4;
        const float4 sre = ld4(ps), sim = ld4(ps + dc), rre = ld4(pr), rim = ld4(pr + dc);
        u_re = make_float4(sre.x * rre.x - sim.x * rim.x, sre.y * rre.y - sim.y * rim.y,
                           sre.z * rre.z - sim.z * rim.z, sre.w * rre.w - sim.w * rim.w);
        u_im = make_float4(sim.x * rre.x + sre.x * rim.x, sim.y * rre.y + sre.y * rim.y,
                           sim.z * rre.z + sre.z * rim.z, sim.w * rre.w + sre.w * rim.w);
      }
      float* d = Ut + c4 * US + b;
      d[0] = u_re.x, d[US] = u_re.y, d[2 * US] = u_re.z, d[3 * US] = u_re.w;
      d += 32 * US;
      d[0] = u_im.x, d[US] = u_im.y, d[2 * US] = u_im.z, d[3 * US] = u_im.w;
    }
    // Nt: (t >> 3) & 1 picks the half, row t >> 4 of 16 per pass
    const int half = (t >> 3) & 1;
    for (int j = t >> 4; j < Mp; j += 16) {
      float4 v = zero4();
      if (j < M && col_ok)
        v = ld4(row_ref<SLAB>(p, ROLE_N, (int64_t)c * M + j).in + half * dc + k0 + c4);
      float* d = Nt + (half * 32 + c4) * NS + j;
      d[0] = v.x, d[NS] = v.y, d[2 * NS] = v.z, d[3 * NS] = v.w;
    }
    for (int i = t; i < Cp * Mp; i += CT) {
      const int b = i / Mp, j = i - b * Mp;
      Gl[b * NS + j] = (b < Cc && j < M) ? p.G[(int64_t)(b0 + b) * M + j] : 0.f;
    }
  }
  __syncthreads();

  // ---- A = G N, then g_s, g_r, g_o of (positive, complex column), held in
  // registers until every wave has read its embeddings
  const int ct = wave & 1;
  const int kcol = k0 + 16 * ct + x;  // this lane's complex column
  float gs_re[2][4], gs_im[2][4], gr_re[2][4], gr_im[2][4], go_re[2][4], go_im[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int mt = (wave >> 1) + 2 * h;
    f32x4 a_re = {0.f, 0.f, 0.f, 0.f}, a_im = {0.f, 0.f, 0.f, 0.f};
    if (16 * mt < Cc) {  // the same for the whole wave
      const float* ga = Gl + (16 * mt + x) * NS + kk;
      const float* nre = Nt + (16 * ct + x) * NS + kk;
      const float* nim = nre + 32 * NS;
      for (int j = 0; j < Mp; j += 4) {
        const float g = ga[j];
        a_re = __builtin_amdgcn_mfma_f32_16x16x4f32(g, nre[j], a_re, 0, 0, 0);
        a_im = __builtin_amdgcn_mfma_f32_16x16x4f32(g, nim[j], a_im, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = 16 * mt + 4 * kk + r;
      gs_re[h][r] = gs_im[h][r] = gr_re[h][r] = gr_im[h][r] = go_re[h][r] = go_im[h][r] = 0.f;
      if (b >= Cc || kcol >= dc) continue;
      const float* ps = row_ref<SLAB>(p, ROLE_S, b0 + b).in;
      const float* pr = row_ref<SLAB>(p, ROLE_R, b0 + b).in;
      const float* po = row_ref<SLAB>(p, ROLE_O, b0 + b).in;
      const float g0 = p.g0[b0 + b];
      const float s_re = ps[kcol], s_im = ps[dc + kcol], r_re = pr[kcol], r_im = pr[dc + kcol];
      const float are = a_re[r] + g0 * po[kcol], aim = a_im[r] + g0 * po[dc + kcol];
      gs_re[h][r] = are * r_re + aim * r_im;
      gs_im[h][r] = aim * r_re - are * r_im;
      gr_re[h][r] = are * s_re + aim * s_im;
      gr_im[h][r] = aim * s_re - are * s_im;
      go_re[h][r] = g0 * (s_re * r_re - s_im * r_im);
      go_im[h][r] = g0 * (s_im * r_re + s_re * r_im);
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = 16 * ((wave >> 1) + 2 * h) + 4 * kk + r;
      if (b >= Cc || kcol >= dc) continue;
      const RowRef rs = row_ref<SLAB>(p, ROLE_S, b0 + b);
      write_elem<SLAB>(rs, kcol, D, gs_re[h][r], p.lr, p.eps);
      write_elem<SLAB>(rs, dc + kcol, D, gs_im[h][r], p.lr, p.eps);
      const RowRef rr = row_ref<SLAB>(p, ROLE_R, b0 + b);
      write_elem<SLAB>(rr, kcol, D, gr_re[h][r], p.lr, p.eps);
      write_elem<SLAB>(rr, dc + kcol, D, gr_im[h][r], p.lr, p.eps);
      const RowRef ro = row_ref<SLAB>(p, ROLE_O, b0 + b);
      write_elem<SLAB>(ro, kcol, D, go_re[h][r], p.lr, p.eps);
      write_elem<SLAB>(ro, dc + kcol, D, go_im[h][r], p.lr, p.eps);
    }
  }

  // ---- dN = G^T U: wave w has columns 16 * w .. of the 64 (0..31 re, 32..63 im)
  const int ncol = (wave >> 1) * dc + k0 + 16 * (wave & 1) + x;  // float column of the row
  const bool ncol_ok = k0 + 16 * (wave & 1) + x < dc;
  const float* ub = Ut + (16 * wave + x) * US + kk;
  for (int jt = 0; 16 * jt < M; ++jt) {
    f32x4 dn = {0.f, 0.f, 0.f, 0.f};
    const float* gt = Gl + kk * NS + 16 * jt + x;
    for (int b = 0; b < Cp; b += 4)
      dn = __builtin_amdgcn_mfma_f32_16x16x4f32(gt[b * NS], ub[b], dn, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 16 * jt + 4 * kk + r;
      if (j >= M || !ncol_ok) continue;
      write_elem<SLAB>(row_ref<SLAB>(p, ROLE_N, (int64_t)c * M + j), ncol, D, dn[r], p.lr, p.eps);
    }
  }
}

inline int round16(int v) { return (v + 15) / 16 * 16; }

template <bool SLAB>
void launch_chunk(ChunkArgs p, float* scratch, void* stream) {
  if (p.B < 1) return;
  const int64_t B = p.B;
  p.G = scratch;
  p.g0 = scratch + B * p.M;
  p.lossp = p.g0 + B;
  const int n_chunks = (p.B + p.C - 1) / p.C;
  const int mblocks = (p.M + SB - 1) / SB;
  const int cblocks = (p.D / 2 + UW - 1) / UW;
  const int Cp = round16(std::min(p.C, p.B)), Mp = round16(p.M);
  const size_t lds = kge_chunk_update_lds_bytes(std::min(p.C, p.B), p.M);
  hipLaunchKernelGGL(k_chunk_scores<SLAB>, dim3((unsigned)((int64_t)n_chunks * mblocks)),
                     dim3(CT), 0, (hipStream_t)stream, p, mblocks);
  hipLaunchKernelGGL(k_chunk_update<SLAB>, dim3((unsigned)((int64_t)n_chunks * cblocks)),
                     dim3(CT), lds, (hipStream_t)stream, p, cblocks, Cp, Mp);
}

}  // namespace

size_t kge_chunk_update_lds_bytes(int C, int M) {
  const int Cp = round16(C), Mp = round16(M);
  return ((size_t)64 * (Cp + 4) + (size_t)(64 + Cp) * (Mp + 4)) * sizeof(float);
}

void kge_complex_step_chunk_gpu(const float* s, const float* r, const float* o, const float* neg,
                                float* ds, float* dr, float* do_, float* dneg, float* loss,
                                float* scratch, int B, int C, int M, int D, float lr, float eps,
                                void* stream) {
  ChunkArgs p{};
  p.in[ROLE_S] = s, p.in[ROLE_R] = r, p.in[ROLE_O] = o, p.in[ROLE_N] = neg;
  p.out[ROLE_S] = ds, p.out[ROLE_R] = dr, p.out[ROLE_O] = do_, p.out[ROLE_N] = dneg;
  p.loss = loss;
  p.B = B, p.C = C, p.M = M, p.D = D, p.lr = lr, p.eps = eps;
  launch_chunk<false>(p, scratch, stream);
}

void kge_complex_step_chunk_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                      const int64_t* keys_o, const int64_t* keys_neg, float* loss,
                                      float* scratch, int B, int C, int M, int D, int32_t plen,
                                      int world, float lr, float eps, void* stream,
                                      const uint32_t* bits) {
  ChunkArgs p{};
  p.slab = slab;
  p.keys[ROLE_S] = keys_s, p.keys[ROLE_R] = keys_r, p.keys[ROLE_O] = keys_o;
  p.keys[ROLE_N] = keys_neg;
  p.bits = bits, p.plen = plen, p.world = world;
  p.loss = loss;
  p.B = B, p.C = C, p.M = M, p.D = D, p.lr = lr, p.eps = eps;
  launch_chunk<true>(p, scratch, stream);
}

}  // namespace adapm
