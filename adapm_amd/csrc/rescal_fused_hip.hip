// Fused slab-direct RESCAL step (contract: kernels.h, rescal_step_fused_gpu).
//   k_rescal_fused_u    U = S_g R_g, the s rows gathered from the slab; leaves
//                       their embedding halves in Sc
//   k_rescal_fused_mid  one wave per triple: scores, W, AdaGrad of o and o'_j
//                       in place
//   k_rescal_fused_ds   s += AdaGrad(W R_g^T), written from the accumulators
//   k_rescal_fused_dr   R_g += AdaGrad(Sc_g^T W_g), likewise
//
// The three products share one tile body (fused_tile). A workgroup of 4 waves
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
};

template <int NT>
struct TileLds {
  float a[16][KP];
  float b[64 * NT][KP];
};

enum { MODE_U = 0, MODE_DS = 1, MODE_DR = 2 };

// One 16 x D output tile of group g, rows m0.. of the product
//   MODE_U   U  = S R      M = Bg, K = D   A gathered from the slab
//   MODE_DS  dS = W R^T    M = Bg, K = D   A = W rows
//   MODE_DR  dR = Sc^T W   M = D,  K = Bg  A = Sc columns
// followed by the mode's epilogue.
template <int NT, int MODE>
__device__ inline void fused_tile(const FusedArgs& p, int g, int m0) {
  constexpr int NBUF = NT <= 3 ? 2 : 1;
  __shared__ TileLds<NT> lds[NBUF];
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int D = p.D;
  const int s0 = p.starts[g];
  const int Bg = p.starts[g + 1] - s0;
  const int M = MODE == MODE_DR ? D : Bg;
  const int K = MODE == MODE_DR ? Bg : D;
  float* Rg = p.slab + p.offs_rg[g];

  // A: 16 rows x 32 k = 128 float4, one for each of the first 128 threads.
  // MODE_U / MODE_DS: thread -> (row t >> 3, k 4 * (t & 7)), along k.
  // MODE_DR: thread -> (sample t >> 2, rows 4 * (t & 3)), along the row of Sc;
  // stored transposed.
  const bool a_thread = t < 128;
  const int ar = MODE == MODE_DR ? (t & 3) * 4 : t >> 3;  // first tile row of this thread
  const int ak = MODE == MODE_DR ? t >> 2 : (t & 7) * 4;  // first k within the chunk
  const float* a_src = nullptr;
  float* sc_dst = nullptr;
  if (a_thread) {
    if (MODE == MODE_DR) {
      if (m0 + ar < M) a_src = p.Sc + (int64_t)(s0 + ak) * D + m0 + ar;
    } else if (m0 + ar < M) {
      const int64_t b = s0 + m0 + ar;
      a_src = MODE == MODE_U ? p.slab + p.offs_s[b] + ak : p.W + b * D + ak;
      if (MODE == MODE_U) sc_dst = p.Sc + b * D + ak;
    }
  }
  // B: 64*NT columns x 32 k = 512*NT float4, 2*NT per thread.
  // Source row-major [k][n] (MODE_U: R, MODE_DR: W of the group): float4
  // along n, lanes along k so that the 4 transposed LDS stores of a wave hit
  // 32 consecutive banks. MODE_DS reads R[n][k] along k and stores float4.
  const float* b_src = MODE == MODE_DR ? p.W + (int64_t)s0 * D : Rg;

  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 rb[2 * NT];
  auto load_chunk = [&](int k0) {
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a_src) {
      if (MODE == MODE_DR) {
        if (k0 + ak < K) ra = ld4(a_src + (int64_t)k0 * D);
      } else if (k0 + ak < K) {
        ra = ld4(a_src + k0);
        if (MODE == MODE_U) *reinterpret_cast<float4*>(sc_dst + k0) = ra;
      }
    }
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) {
      const int idx = t + i * FT;
      rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (MODE == MODE_DS) {
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
      if (MODE == MODE_DR) {
        L.a[ar][ak] = ra.x, L.a[ar + 1][ak] = ra.y, L.a[ar + 2][ak] = ra.z, L.a[ar + 3][ak] = ra.w;
      } else {
        *reinterpret_cast<float4*>(&L.a[ar][ak]) = ra;
      }
    }
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) {
      const int idx = t + i * FT;
      if (MODE == MODE_DS) {
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
  const int nchunks = (K + KC - 1) / KC;
  load_chunk(0);
  store_chunk(lds[0]);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const bool more = c + 1 < nchunks;
    if (more) load_chunk((c + 1) * KC);
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
  if (MODE == MODE_DS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + kk * 4 + r;
      row_off[r] = row < M ? p.offs_s[s0 + row] : 0;
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
      } else if (MODE == MODE_DS) {
        float* e = p.slab + row_off[r] + col;
        rf_slab_adagrad(e, e + D, gr, e[D], p.lr, p.eps);
      } else {
        const int64_t dd = (int64_t)D * D;
        float* e = Rg + (int64_t)row * D + col;
        rf_slab_adagrad(e, e + dd, gr, e[dd], p.lr, p.eps);
      }
    }
  }
}

template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_fused_u(FusedArgs p) {
  fused_tile<NT, MODE_U>(p, p.tiles[2 * blockIdx.x], p.tiles[2 * blockIdx.x + 1]);
}

template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_fused_ds(FusedArgs p) {
  fused_tile<NT, MODE_DS>(p, p.tiles[2 * blockIdx.x], p.tiles[2 * blockIdx.x + 1]);
}

// workgroup (g, i): rows 16 * i.. of R_g
template <int NT>
__global__ void __launch_bounds__(FT) k_rescal_fused_dr(FusedArgs p, int mtiles) {
  fused_tile<NT, MODE_DR>(p, blockIdx.x / mtiles, (blockIdx.x % mtiles) * 16);
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

}  // namespace adapm
