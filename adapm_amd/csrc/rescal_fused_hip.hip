// Fused slab-direct RESCAL step (contract: kernels.h, rescal_step_fused_gpu).
//   k_rescal_fused_u    U = S_g R_g, the s rows gathered from the slab; leaves
//                       their embedding halves in Sc
//   k_rescal_fused_mid  one wave per triple: scores, W, AdaGrad of o and o'_j
//                       in place
//   k_rescal_fused_ds   s += AdaGrad(W R_g^T), written from the accumulators
//   k_rescal_fused_dr   R_g += AdaGrad(Sc_g^T W_g), likewise
// and the two-sided step (contract: kernels.h, rescal_step_sides_fused_gpu),
// again four launches:
//   k_rescal_sides_fused_uv   U as above and V = O_g R_g^T, the o rows gathered
//                             into Oc; the product is chosen per workgroup
//   k_rescal_sides_fused_mid  one wave per triple: object pass against u (the
//                             positive o scored, not written), subject pass
//                             against v; W, Z, c0, loss
//   k_rescal_sides_fused_dso  s += AdaGrad(W R_g^T + gamma_e Sc) and
//                             o += AdaGrad(c0 U + Z R_g + gamma_e Oc)
//   k_rescal_sides_fused_dr   R_g += AdaGrad(Sc_g^T W_g + Z_g^T Oc_g +
//                             gamma_r Bg R_g), one GEMM over K = 2 Bg
//
// All the products share one tile body (fused_tile). A workgroup of 4 waves
// owns 16 rows of the output and ALL its columns: wave w holds NT accumulators
// of v_mfma_f32_16x16x4_f32 for the columns 64*j + 16*w + (lane & 15), so the
// A tile (for U: 16 rows gathered through their offsets) is fetched once per
// K-chunk, not once per 64-column strip. A and B are staged in LDS per
// K-chunk of 32 as la[row][k] and lb[col][k], rows padded to 36 floats: they
// stay 16-byte aligned and 8 consecutive rows start in 8 different groups of
// 4 banks. The MFMA lane (x = lane & 15, kk = lane >> 4) reads
// its 8 k of a chunk as two float4, k = 8*kk + i for MFMA i: any split of a
// chunk's k over the 8 MFMAs gives the same sum as long as A and B agree.
// The next chunk's global loads are issued before the current chunk's MFMAs
// and land in registers; with two LDS buffers (NT <= 3, under 64 KB) a chunk
// costs one barrier, with one buffer (NT = 4) two.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace adapm {
namespace {

constexpr int FT = 256;  // threads per workgroup (4 waves)
constexpr int KC = 32;   // K-chunk
constexpr int KP = KC + 4;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// adagrad_delta of kernels_hip.hip, repeated (kernels.h says why)
__device__ inline float rf_adagrad_delta(float g, float acc, float lr, float eps) {
  float G = acc + g * g;
  return -lr * g * __frsqrt_rn(G + eps);
}

// One element's AdaGrad update on the slab, as slab_adagrad(shared = true).
__device__ inline void rf_slab_adagrad(float* p_emb, float* p_acc, float g, float acc, float lr,
                                       float eps) {
  atomicAdd(p_emb, rf_adagrad_delta(g, acc, lr, eps));
  atomicAdd(p_acc, g * g);
}

// k_rescal_mid's softplus
__device__ inline float rf_softplus(float x) {
  return x > 20.f ? x : __logf(1.f + __expf(x));
}

// softplus1pf of kernels_hip.hip, repeated: log(1 + exp(x)) that keeps its
// relative accuracy where exp(x) is small (log1p as its series below 0.01);
// the sides steps sum up to 1 + N + NS terms (docs/PARITY.md, 2.5).
__device__ inline float rf_softplus1pf(float x) {
  if (x > 20.f) return x;
  float t = __expf(x);
  return t < 0.01f ? t * (1.f - t * (0.5f - t * (1.f / 3.f))) : __logf(1.f + t);
}

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

struct FusedArgs {
  float* slab;
  const int64_t* offs_s;   // [B]
  const int64_t* offs_rg;  // [G]
  const int32_t* starts;   // [G + 1]
  const int32_t* tiles;    // [T][2]: group, first row of the tile within the group
  float* U;                // [B][D]
  float* W;                // [B][D]
  float* Sc;               // [B][D]
  int D;
  float lr, eps;
  // the two-sided step only
  const int64_t* offs_o;  // [B]
  float* V;               // [B][D]
  float* Z;               // [B][D]
  float* Oc;              // [B][D]
  const float* c0;        // [B]
  float gamma_e, gamma_r;
};

template <int NT>
struct TileLds {
  float a[16][KP];
  float b[64 * NT][KP];
};

template <int NT>
constexpr int tile_bufs() { return NT <= 3 ? 2 : 1; }

enum { MODE_U = 0, MODE_DS = 1, MODE_DR = 2, MODE_V = 3, MODE_DS2 = 4, MODE_DO = 5, MODE_DR2 = 6 };

// One 16 x D output tile of group g, rows m0.. of the product
//   MODE_U    U  = S R      M = Bg, K = D   A gathered from the slab (s -> Sc)
//   MODE_DS   dS = W R^T    M = Bg, K = D   A = W rows
//   MODE_DR   dR = Sc^T W   M = D,  K = Bg  A = Sc columns
// and for the two-sided step
//   MODE_V    V  = O R^T    M = Bg, K = D   A gathered from the slab (o -> Oc)
//   MODE_DS2  dS = W R^T + gamma_e Sc
//   MODE_DO   dO = Z R + c0 U + gamma_e Oc  A = Z rows
//   MODE_DR2  dR = Sc^T W + Z^T Oc + gamma_r Bg R, one product over K = 2 Bg:
//             the chunks of Bg come from (Sc, W), then the sources are
//             swapped and the chunks of Bg come again from (Z, Oc), so each
//             half's tail chunk is zero-padded on its own
// followed by the mode's epilogue. `lds` is the kernel's one tile buffer.
// PAIRED marks the body of a kernel that chooses between two products: it
// keeps k_rescal_sides_fused_uv from sharing k_rescal_fused_u's instantiation,
// whose inlining (and with it the register allocation) a second caller changes.
template <int NT, int MODE, bool PAIRED = false>
__device__ inline void fused_tile(const FusedArgs& p, int g, int m0,
                                  TileLds<NT> (&lds)[tile_bufs<NT>()]) {
  constexpr int NBUF = tile_bufs<NT>();
  constexpr bool IS_DR = MODE == MODE_DR || MODE == MODE_DR2;
  constexpr bool GATHER = MODE == MODE_U || MODE == MODE_V;
  // B staged as MODE_DS does: R[n][k] read along k, float4 LDS stores
  constexpr bool B_ALONG_K = MODE == MODE_DS || MODE == MODE_DS2 || MODE == MODE_V;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int D = p.D;
  const int s0 = p.starts[g];
  const int Bg = p.starts[g + 1] - s0;
  const int M = IS_DR ? D : Bg;
  const int K = IS_DR ? Bg : D;
  float* Rg = p.slab + p.offs_rg[g];

  // A: 16 rows x 32 k = 128 float4, one for each of the first 128 threads.
  // MODE_U / MODE_DS: thread -> (row t >> 3, k 4 * (t & 7)), along k.
  // MODE_DR: thread -> (sample t >> 2, rows 4 * (t & 3)), along the row of Sc;
  // stored transposed.
  const bool a_thread = t < 128;
  const int ar = IS_DR ? (t & 3) * 4 : t >> 3;  // first tile row of this thread
  const int ak = IS_DR ? t >> 2 : (t & 7) * 4;  // first k within the chunk
  const float* a_src = nullptr;
  const float* a_src2 = nullptr;  // MODE_DR2: the second half's Z
  float* sc_dst = nullptr;
  if (a_thread) {
    if (IS_DR) {
      if (m0 + ar < M) {
        a_src = p.Sc + (int64_t)(s0 + ak) * D + m0 + ar;
        if (MODE == MODE_DR2) a_src2 = p.Z + (int64_t)(s0 + ak) * D + m0 + ar;
      }
    } else if (m0 + ar < M) {
      const int64_t b = s0 + m0 + ar;
      if (MODE == MODE_U) {
        a_src = p.slab + p.offs_s[b] + ak;
        sc_dst = p.Sc + b * D + ak;
      } else if (MODE == MODE_V) {
        a_src = p.slab + p.offs_o[b] + ak;
        sc_dst = p.Oc + b * D + ak;
      } else {
        a_src = (MODE == MODE_DO ? p.Z : p.W) + b * D + ak;
      }
    }
  }
  // B: 64*NT columns x 32 k = 512*NT float4, 2*NT per thread.
  // Source row-major [k][n] (MODE_U, MODE_DO: R, MODE_DR: W of the group,
  // MODE_DR2: W, then Oc): float4 along n, lanes along k so that the 4
  // transposed LDS stores of a wave hit 32 consecutive banks. MODE_DS,
  // MODE_DS2 and MODE_V read R[n][k] along k and store float4.
  const float* b_src = IS_DR ? p.W + (int64_t)s0 * D : Rg;
  const float* b_src2 = MODE == MODE_DR2 ? p.Oc + (int64_t)s0 * D : nullptr;

  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 rb[2 * NT];
  auto load_chunk = [&](int k0) {
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a_src) {
      if (IS_DR) {
        if (k0 + ak < K) ra = ld4(a_src + (int64_t)k0 * D);
      } else if (k0 + ak < K) {
        ra = ld4(a_src + k0);
        if (GATHER) *reinterpret_cast<float4*>(sc_dst + k0) = ra;
      }
    }
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) {
      const int idx = t + i * FT;
      rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (B_ALONG_K) {
        const int n = idx >> 3, k = k0 + (idx & 7) * 4;
        if (n < D && k < K) rb[i] = ld4(b_src + (int64_t)n * D + k);
      } else {
        const int k = k0 + (idx & 31), n = (idx >> 5) * 4;
        if (n < D && k < K) rb[i] = ld4(b_src + (int64_t)k * D + n);
      }
    }
  };
  auto store_chunk = [&](TileLds<NT>& L) {
    if (a_thread) {
      if (IS_DR) {
        L.a[ar][ak] = ra.x, L.a[ar + 1][ak] = ra.y, L.a[ar + 2][ak] = ra.z, L.a[ar + 3][ak] = ra.w;
      } else {
        *reinterpret_cast<float4*>(&L.a[ar][ak]) = ra;
      }
    }
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) {
      const int idx = t + i * FT;
      if (B_ALONG_K) {
        *reinterpret_cast<float4*>(&L.b[idx >> 3][(idx & 7) * 4]) = rb[i];
      } else {
        const int k = idx & 31, n = (idx >> 5) * 4;
        L.b[n][k] = rb[i].x, L.b[n + 1][k] = rb[i].y, L.b[n + 2][k] = rb[i].z;
        L.b[n + 3][k] = rb[i].w;
      }
    }
  };

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};

  const int x = lane & 15, kk = lane >> 4;
  const int hchunks = (K + KC - 1) / KC;
  const int nchunks = MODE == MODE_DR2 ? 2 * hchunks : hchunks;
  load_chunk(0);
  store_chunk(lds[0]);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const bool more = c + 1 < nchunks;
    if (MODE == MODE_DR2) {
      if (c + 1 == hchunks) a_src = a_src2, b_src = b_src2;  // the second half
      if (more) load_chunk((c + 1 < hchunks ? c + 1 : c + 1 - hchunks) * KC);
    } else if (more) {
      load_chunk((c + 1) * KC);
    }
    const TileLds<NT>& L = lds[c % NBUF];
    const float4 a0 = ld4(&L.a[x][kk * 8]), a1 = ld4(&L.a[x][kk * 8 + 4]);
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = 64 * j + 16 * wave;  // the same for a whole wave
      if (n >= D) continue;
      const float4 b0 = ld4(&L.b[n + x][kk * 8]), b1 = ld4(&L.b[n + x][kk * 8 + 4]);
      const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc[j], 0, 0, 0);
    }
    if (NBUF == 1) __syncthreads();  // all reads of the one buffer done
    if (more) store_chunk(lds[(c + 1) % NBUF]);
    __syncthreads();
  }

  // accumulator element r of lane: row (lane >> 4) * 4 + r, column n + x
  int64_t row_off[4];
  float row_c0[4];  // MODE_DO
  if (MODE == MODE_DS || MODE == MODE_DS2 || MODE == MODE_DO) {
    const int64_t* offs = MODE == MODE_DO ? p.offs_o : p.offs_s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + kk * 4 + r;
      row_off[r] = row < M ? offs[s0 + row] : 0;
      if (MODE == MODE_DO) row_c0[r] = row < M ? p.c0[s0 + row] : 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = 64 * j + 16 * wave + x;
    if (col >= D) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + kk * 4 + r;
      if (row >= M) continue;
      const float gr = acc[j][r];
      if (MODE == MODE_U) {
        p.U[(int64_t)(s0 + row) * D + col] = gr;
      } else if (MODE == MODE_V) {
        p.V[(int64_t)(s0 + row) * D + col] = gr;
      } else if (MODE == MODE_DS) {
        float* e = p.slab + row_off[r] + col;
        rf_slab_adagrad(e, e + D, gr, e[D], p.lr, p.eps);
      } else if (MODE == MODE_DS2 || MODE == MODE_DO) {
        const int64_t i = (int64_t)(s0 + row) * D + col;
        float* e = p.slab + row_off[r] + col;
        const float gs = MODE == MODE_DS2 ? gr + p.gamma_e * p.Sc[i]
                                          : row_c0[r] * p.U[i] + gr + p.gamma_e * p.Oc[i];
        rf_slab_adagrad(e, e + D, gs, e[D], p.lr, p.eps);
      } else {
        const int64_t dd = (int64_t)D * D;
        float* e = Rg + (int64_t)row * D + col;
        // MODE_DR2: each of the group's Bg positives adds gamma_r R
        const float gs = MODE == MODE_DR2 ? gr + p.gamma_r * (float)Bg * e[0] : gr;
        rf_slab_adagrad(e, e + dd, gs, e[dd], p.lr, p.eps);
      }
    }
  }
}

template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_fused_u(FusedArgs p) {
  __shared__ TileLds<NT> lds[tile_bufs<NT>()];
  fused_tile<NT, MODE_U>(p, p.tiles[2 * blockIdx.x], p.tiles[2 * blockIdx.x + 1], lds);
}

template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_fused_ds(FusedArgs p) {
  __shared__ TileLds<NT> lds[tile_bufs<NT>()];
  fused_tile<NT, MODE_DS>(p, p.tiles[2 * blockIdx.x], p.tiles[2 * blockIdx.x + 1], lds);
}

// workgroup (g, i): rows 16 * i.. of R_g
template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_fused_dr(FusedArgs p, int mtiles) {
  __shared__ TileLds<NT> lds[tile_bufs<NT>()];
  fused_tile<NT, MODE_DR>(p, blockIdx.x / mtiles, (blockIdx.x % mtiles) * 16, lds);
}

// One wave per triple, four triples per workgroup, grid-stride. Lane l holds
// u[64*j + l], j < NT, and the same columns of w and of the candidate row in
// registers; the score is a butterfly over the wave, so the kernel has no LDS
// and no barrier. The next candidate's row is loaded before the current one
// is scored.
template <int NT>
__global__ void __launch_bounds__(FT)
k_rescal_fused_mid(float* __restrict__ slab, const int64_t* __restrict__ offs_o,
                   const int64_t* __restrict__ offs_neg, const float* __restrict__ U,
                   float* __restrict__ W, float* __restrict__ loss, int B, int N, int D, float lr,
                   float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
    float u[NT], w[NT], e[NT], a[NT], ne[NT], na[NT];
    float* row = slab + offs_o[b];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = 64 * j + lane;
      const bool ok = col < D;
      u[j] = ok ? U[b * D + col] : 0.f;
      e[j] = ok ? row[col] : 0.f;
      a[j] = ok ? row[D + col] : 0.f;
      w[j] = ne[j] = na[j] = 0.f;
    }
    float lsum = 0.f;
    for (int c = 0; c <= N; ++c) {
      float* nrow = row;
      if (c < N) {
        nrow = slab + offs_neg[b * N + c];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int col = 64 * j + lane;
          if (col < D) ne[j] = nrow[col], na[j] = nrow[D + col];
        }
      }
      const float y = c == 0 ? 1.f : -1.f;
      float psi = 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j) psi += u[j] * e[j];
      for (int off = 32; off > 0; off >>= 1) psi += __shfl_xor(psi, off, 64);
      const float cc = -y / (1.f + __expf(y * psi));
      lsum += rf_softplus(-y * psi);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = 64 * j + lane;
        if (col >= D) continue;
        w[j] += cc * e[j];
        rf_slab_adagrad(row + col, row + D + col, cc * u[j], a[j], lr, eps);
      }
      row = nrow;
#pragma unroll
      for (int j = 0; j < NT; ++j) e[j] = ne[j], a[j] = na[j];
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = 64 * j + lane;
      if (col < D) W[b * D + col] = w[j];
    }
    if (lane == 0) loss[b] = lsum;
  }
}

// ---------------------------------------------------------------- two-sided step

// workgroups [0, n_tiles): U; [n_tiles, 2 n_tiles): V over the same tiles
template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_sides_fused_uv(FusedArgs p, int n_tiles) {
  __shared__ TileLds<NT> lds[tile_bufs<NT>()];
  const bool second = (int)blockIdx.x >= n_tiles;
  const int tile = blockIdx.x - (second ? n_tiles : 0);
  const int g = p.tiles[2 * tile], m0 = p.tiles[2 * tile + 1];
  if (second) fused_tile<NT, MODE_V, true>(p, g, m0, lds);
  else fused_tile<NT, MODE_U, true>(p, g, m0, lds);
}

// workgroups [0, n_tiles): ds; [n_tiles, 2 n_tiles): do
template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_sides_fused_dso(FusedArgs p, int n_tiles) {
  __shared__ TileLds<NT> lds[tile_bufs<NT>()];
  const bool second = (int)blockIdx.x >= n_tiles;
  const int tile = blockIdx.x - (second ? n_tiles : 0);
  const int g = p.tiles[2 * tile], m0 = p.tiles[2 * tile + 1];
  if (second) fused_tile<NT, MODE_DO, true>(p, g, m0, lds);
  else fused_tile<NT, MODE_DS2, true>(p, g, m0, lds);
}

template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_sides_fused_dr(FusedArgs p, int mtiles) {
  __shared__ TileLds<NT> lds[tile_bufs<NT>()];
  fused_tile<NT, MODE_DR2>(p, blockIdx.x / mtiles, (blockIdx.x % mtiles) * 16, lds);
}

constexpr int MID_GRID_CAP = 8192;  // workgroups of 4 triples

// k_rescal_fused_mid's shape (a wave per triple, lane l on columns 64*j + l,
// no LDS, no barrier, the next row loaded before the current one is scored),
// run twice. Object pass: x = u; the positive o is scored and enters w but is
// NOT written (R^T z and gamma_e o are still to come, k_rescal_sides_fused_dso
// writes it); every o'_j gets c_j u in place. Subject pass: the same registers
// with x = v and the sum z; every s'_j gets a_j v in place.
template <int NT>
__global__ void __launch_bounds__(FT)
k_rescal_sides_fused_mid(float* __restrict__ slab, const int64_t* __restrict__ offs_o,
                         const int64_t* __restrict__ offs_no, const int64_t* __restrict__ offs_ns,
                         const float* __restrict__ U, const float* __restrict__ V,
                         float* __restrict__ W, float* __restrict__ Z, float* __restrict__ c0,
                         float* __restrict__ loss, int B, int N, int NS, int D, float lr,
                         float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < B; b += (int64_t)gridDim.x * 4) {
    float x[NT], sum[NT], e[NT], a[NT], ne[NT], na[NT];
    float lsum = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
      const float* X = (pass == 0 ? U : V) + b * D;
      const int64_t* offs = pass == 0 ? offs_no + b * N : offs_ns + b * NS;
      // candidates: pass 0 the positive and N negatives, pass 1 NS negatives
      const int first = pass == 0 ? -1 : 0, n = pass == 0 ? N : NS;
      float* row = nullptr;
      if (pass == 0) row = slab + offs_o[b];
      else if (NS > 0) row = slab + offs[0];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = 64 * j + lane;
        const bool ok = col < D;
        x[j] = ok ? X[col] : 0.f;
        e[j] = ok && row ? row[col] : 0.f;
        a[j] = ok && row && pass == 1 ? row[D + col] : 0.f;  // the positive o is not written
        sum[j] = ne[j] = na[j] = 0.f;
      }
      for (int c = first; c < n; ++c) {
        float* nrow = row;
        if (c + 1 < n) {
          nrow = slab + offs[c + 1];
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const int col = 64 * j + lane;
            if (col < D) ne[j] = nrow[col], na[j] = nrow[D + col];
          }
        }
        const float y = c < 0 ? 1.f : -1.f;
        float psi = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) psi += x[j] * e[j];
        for (int off = 32; off > 0; off >>= 1) psi += __shfl_xor(psi, off, 64);
        const float cc = -y / (1.f + __expf(y * psi));
        lsum += rf_softplus1pf(-y * psi);
        if (c < 0 && lane == 0) c0[b] = cc;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int col = 64 * j + lane;
          if (col >= D) continue;
          sum[j] += cc * e[j];
          if (c >= 0) rf_slab_adagrad(row + col, row + D + col, cc * x[j], a[j], lr, eps);
        }
        row = nrow;
#pragma unroll
        for (int j = 0; j < NT; ++j) e[j] = ne[j], a[j] = na[j];
      }
      float* out = (pass == 0 ? W : Z) + b * D;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = 64 * j + lane;
        if (col < D) out[col] = sum[j];
      }
    }
    if (lane == 0) loss[b] = lsum;
  }
}

template <int NT>
void launch_sides_step(const FusedArgs& p, const int64_t* offs_no, const int64_t* offs_ns,
                       float* c0, float* loss, int B, int G, int N, int NS, int n_tiles,
                       hipStream_t st) {
  const int D = p.D;
  const int mtiles = (D + 15) / 16;
  hipLaunchKernelGGL(k_rescal_sides_fused_uv<NT>, dim3(2 * n_tiles), dim3(FT), 0, st, p, n_tiles);
  hipLaunchKernelGGL(k_rescal_sides_fused_mid<NT>, dim3(std::min((B + 3) / 4, MID_GRID_CAP)),
                     dim3(FT), 0, st, p.slab, p.offs_o, offs_no, offs_ns, p.U, p.V, p.W, p.Z, c0,
                     loss, B, N, NS, D, p.lr, p.eps);
  hipLaunchKernelGGL(k_rescal_sides_fused_dso<NT>, dim3(2 * n_tiles), dim3(FT), 0, st, p,
                     n_tiles);
  hipLaunchKernelGGL(k_rescal_sides_fused_dr<NT>, dim3(G * mtiles), dim3(FT), 0, st, p, mtiles);
}

template <int NT>
void launch_step(const FusedArgs& p, const int64_t* offs_o, const int64_t* offs_neg, float* loss,
                 int B, int G, int N, int n_tiles, hipStream_t st) {
  const int D = p.D;
  const int mtiles = (D + 15) / 16;
  hipLaunchKernelGGL(k_rescal_fused_u<NT>, dim3(n_tiles), dim3(FT), 0, st, p);
  hipLaunchKernelGGL(k_rescal_fused_mid<NT>, dim3(std::min((B + 3) / 4, 8192)), dim3(FT), 0, st,
                     p.slab, offs_o, offs_neg, p.U, p.W, loss, B, N, D, p.lr, p.eps);
  hipLaunchKernelGGL(k_rescal_fused_ds<NT>, dim3(n_tiles), dim3(FT), 0, st, p);
  hipLaunchKernelGGL(k_rescal_fused_dr<NT>, dim3(G * mtiles), dim3(FT), 0, st, p, mtiles);
}

}  // namespace

void rescal_step_fused_gpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                           const int64_t* offs_neg, const int64_t* offs_rg, const int32_t* starts,
                           const int32_t* tiles, int n_tiles, float* U, float* W, float* Sc,
                           float* loss, int B, int G, int N, int D, float lr, float eps,
                           void* stream) {
  if (B < 1 || G < 1 || n_tiles < 1) return;
  const FusedArgs p{slab, offs_s, offs_rg, starts, tiles, U, W, Sc, D, lr, eps};
  auto st = (hipStream_t)stream;
  switch ((D + 63) / 64) {
    case 1: launch_step<1>(p, offs_o, offs_neg, loss, B, G, N, n_tiles, st); break;
    case 2: launch_step<2>(p, offs_o, offs_neg, loss, B, G, N, n_tiles, st); break;
    case 3: launch_step<3>(p, offs_o, offs_neg, loss, B, G, N, n_tiles, st); break;
    default: launch_step<4>(p, offs_o, offs_neg, loss, B, G, N, n_tiles, st); break;
  }
}

void rescal_step_sides_fused_gpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                                 const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                 const int64_t* offs_rg, const int32_t* starts,
                                 const int32_t* tiles, int n_tiles, float* scratch, float* loss,
                                 int B, int G, int N, int NS, int D, float lr, float eps,
                                 float gamma_e, float gamma_r, void* stream) {
  if (B < 1 || G < 1 || n_tiles < 1) return;
  const int64_t bd = (int64_t)B * D;
  float* c0 = scratch + 6 * bd;
  FusedArgs p{slab, offs_s, offs_rg, starts, tiles, scratch, scratch + 2 * bd, scratch + 4 * bd,
              D, lr, eps};
  p.offs_o = offs_o;
  p.V = scratch + bd;
  p.Z = scratch + 3 * bd;
  p.Oc = scratch + 5 * bd;
  p.c0 = c0;
  p.gamma_e = gamma_e;
  p.gamma_r = gamma_r;
  auto st = (hipStream_t)stream;
  switch ((D + 63) / 64) {
    case 1:
      launch_sides_step<1>(p, offs_neg_o, offs_neg_s, c0, loss, B, G, N, NS, n_tiles, st);
      break;
    case 2:
      launch_sides_step<2>(p, offs_neg_o, offs_neg_s, c0, loss, B, G, N, NS, n_tiles, st);
      break;
    case 3:
      launch_sides_step<3>(p, offs_neg_o, offs_neg_s, c0, loss, B, G, N, NS, n_tiles, st);
      break;
    default:
      launch_sides_step<4>(p, offs_neg_o, offs_neg_s, c0, loss, B, G, N, NS, n_tiles, st);
      break;
  }
}

}  // namespace adapm
