// Fused CTR embedding step on the slab's own rows (contract: kernels.h).
//   k_ctr_gather        x[i] = emb half of the row of keys[i]
//   k_ctr_seg_adagrad   one lane group per chunk of the sorted keys: whole
//                       segments get their AdaGrad update, open runs leave a
//                       partial sum in scratch
//   k_ctr_seg_tail      one wave per head of a chunk-spanning segment: joins
//                       the partials, then the AdaGrad update
// No atomics anywhere; every row is written by exactly one lane group.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace adapm {
namespace {

constexpr int CT = 256;  // threads per workgroup
constexpr int WAVE = 64;
constexpr int C = CTR_SEG_CHUNK;

// V consecutive floats of a row in one lane: V = 4 moves as one 16-byte
// access, V = 1 is the any-D, any-alignment mapping.
template <int V>
struct Pack {
  float v[V];
};

template <int V>
__device__ inline Pack<V> ld(const float* p) {
  Pack<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
__device__ inline void st(float* p, const Pack<V>& a) {
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
  else
    *p = a.v[0];
}

template <int V>
__device__ inline void add(Pack<V>& a, const Pack<V>& b) {
#pragma unroll
  for (int q = 0; q < V; ++q) a.v[q] += b.v[q];
}

// identity layout: key k at (k / world) * plen
__device__ inline int64_t row_off(int64_t key, int32_t plen, int world) {
  return (key / world) * (int64_t)plen;
}

// One AdaGrad update of the summed gradient g on V floats of a row, in place:
// `row` points at the embedding floats, their accumulators sit D further on.
template <int V>
__device__ inline void adagrad_row(float* row, int D, const Pack<V>& g, float lr, float eps) {
  Pack<V> emb = ld<V>(row), acc = ld<V>(row + D);
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const float g2 = g.v[q] * g.v[q];
    const float G = acc.v[q] + g2;
    emb.v[q] += -lr * g.v[q] / sqrtf(G + eps);
    acc.v[q] = G;
  }
  st<V>(row, emb);
  st<V>(row + D, acc);
}

// Thread t of the grid moves V floats: column block t % nvec of occurrence
// t / nvec, so consecutive lanes read one row's consecutive floats and write
// x fully coalesced.
template <int V>
__global__ void __launch_bounds__(CT)
k_ctr_gather(const float* __restrict__ slab, const int64_t* __restrict__ keys,
             float* __restrict__ x, int64_t n, int D, int32_t plen, int world) {
  const int nvec = D / V;
  const int64_t total = n * nvec;
  const int64_t stride = (int64_t)gridDim.x * CT;
  for (int64_t t = (int64_t)blockIdx.x * CT + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / nvec;
    const int col = (int)(t - i * nvec) * V;
    st<V>(x + i * D + col, ld<V>(slab + row_off(keys[i], plen, world) + col));
  }
}

// Lane group `threadIdx.x >> lg` of the workgroup (1 << lg lanes) walks chunk
// [a, b) of the sorted keys; lane c0 of the group owns the columns
// [c * V, c * V + V) for c = c0, c0 + lanes, ... (more than one only where a
// row is longer than 64 * V floats: the chunk is then walked once per c).
// The next position's key and occurrence are loaded before this position's
// gradient row is used, so the dependent loads of consecutive positions
// overlap. Reading ks[p + 1] across the chunk's right edge is what tells a run
// that ends with the chunk from one that goes on.
template <int V>
__global__ void __launch_bounds__(CT)
k_ctr_seg_adagrad(float* __restrict__ slab, const int64_t* __restrict__ ks,
                  const int64_t* __restrict__ perm, const float* __restrict__ grad,
                  float* __restrict__ scratch, int64_t n, int D, int32_t plen, int world, int lg,
                  float lr, float eps) {
  const int lanes = 1 << lg;
  const int c0 = threadIdx.x & (lanes - 1);
  const int64_t chunk = (int64_t)blockIdx.x * (CT >> lg) + (threadIdx.x >> lg);
  const int64_t a = chunk * C;
  if (a >= n) return;
  const int64_t b = a + C < n ? a + C : n;
  const int nvec = D / V;
  float* part = scratch + chunk * 2 * D;  // [2][D]: open on the left | only on the right
  for (int c = c0; c < nvec; c += lanes) {
    const int col = c * V;
    int64_t k = ks[a], i = perm[a];
    bool open_left = a > 0 && ks[a - 1] == k;
    Pack<V> acc = {};
    for (int64_t p = a; p < b; ++p) {
      int64_t kn = -1, in = 0;  // keys are >= 0: the array's end closes the run
      if (p + 1 < n) {
        kn = ks[p + 1];
        in = perm[p + 1];
      }
      add<V>(acc, ld<V>(grad + i * D + col));
      if (kn != k) {  // the run ends here
        if (open_left)
          st<V>(part + col, acc);
        else
          adagrad_row<V>(slab + row_off(k, plen, world) + col, D, acc, lr, eps);
        acc = {};
        open_left = false;
      } else if (p + 1 == b) {  // the run goes on past the chunk
        st<V>(part + (open_left ? 0 : D) + col, acc);
      }
      k = kn;
      i = in;
    }
  }
}

// Wave h looks at chunk h. It is the head of a spanning segment if the
// chunk's last run is open on the right but not on the left; every other
// wave leaves at once. The head finds the segment's end (upper bound of its
// key in the sorted array), hence the last chunk `last` whose slot 0 is a
// part of the segment. The wave's G = 64 >> lg lane groups take the chunks
// h + 1 + g, h + 1 + g + G, ... <= last (group 0 starts from the head's own
// slot 1), then a butterfly over the groups adds the G sums: the order of
// additions depends on (h, last, G) alone.
template <int V>
__global__ void __launch_bounds__(CT)
k_ctr_seg_tail(float* __restrict__ slab, const int64_t* __restrict__ ks,
               const float* __restrict__ scratch, int64_t n, int D, int32_t plen, int world,
               int lg, float lr, float eps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t h = (int64_t)blockIdx.x * (CT / WAVE) + (threadIdx.x / WAVE);
  const int64_t e = (h + 1) * C;  // first position of the next chunk
  if (e >= n) return;             // all exits are the same for a whole wave
  const int64_t K = ks[e - 1];
  if (ks[e] != K) return;                        // closed on the right
  if (h > 0 && ks[h * C - 1] == K) return;       // open on the left too: not the head
  int64_t lo = e + 1, hi = n;  // first position in (e, n] whose key is above K
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (ks[mid] <= K)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int64_t last = (lo - 1) / C;
  const int lanes = 1 << lg;
  const int c0 = lane & (lanes - 1);
  const int g = lane >> lg, G = WAVE >> lg;
  const int nvec = D / V;
  for (int cb = 0; cb < nvec; cb += lanes) {
    const int col = (cb + c0) * V;
    const bool active = cb + c0 < nvec;
    Pack<V> acc = {};
    if (active) {
      if (g == 0) acc = ld<V>(scratch + (h * 2 + 1) * D + col);
      for (int64_t j = h + 1 + g; j <= last; j += G)
        add<V>(acc, ld<V>(scratch + j * 2 * D + col));
    }
    for (int off = lanes; off < WAVE; off <<= 1) {
#pragma unroll
      for (int q = 0; q < V; ++q) acc.v[q] += __shfl_xor(acc.v[q], off);
    }
    if (active && g == 0) adagrad_row<V>(slab + row_off(K, plen, world) + col, D, acc, lr, eps);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// log2 of the lanes of a group: the smallest power of two that covers a
// row's nvec column blocks, one wave at the most
inline int group_shift(int nvec) {
  int lg = 0;
  while ((1 << lg) < nvec && (1 << lg) < WAVE) ++lg;
  return lg;
}

}  // namespace

void ctr_gather_fused_gpu(const float* slab, const int64_t* keys, float* x, int64_t n, int D,
                          int32_t plen, int world, void* stream) {
  if (n <= 0) return;
  const bool wide = D % 4 == 0 && plen % 4 == 0 && aligned16(slab) && aligned16(x);
  const int64_t total = n * (wide ? D / 4 : D);
  const dim3 grid((unsigned)std::min<int64_t>((total + CT - 1) / CT, 1 << 20));
  if (wide)
    hipLaunchKernelGGL(k_ctr_gather<4>, grid, dim3(CT), 0, (hipStream_t)stream, slab, keys, x, n,
                       D, plen, world);
  else
    hipLaunchKernelGGL(k_ctr_gather<1>, grid, dim3(CT), 0, (hipStream_t)stream, slab, keys, x, n,
                       D, plen, world);
}

void ctr_update_fused_gpu(float* slab, const int64_t* keys_sorted, const int64_t* perm,
                          const float* grad, float* scratch, int64_t n, int D, int32_t plen,
                          int world, float lr, float eps, void* stream) {
  if (n <= 0) return;
  const bool wide = D % 4 == 0 && plen % 4 == 0 && aligned16(slab) && aligned16(grad) &&
                    aligned16(scratch);
  const int lg = group_shift(wide ? D / 4 : D);
  const int64_t chunks = (n + C - 1) / C;
  const int per_wg = CT >> lg;  // chunks of one workgroup
  const dim3 grid((unsigned)((chunks + per_wg - 1) / per_wg));
  // one wave per chunk; the last chunk cannot be a head
  const dim3 tail_grid((unsigned)((chunks - 1 + CT / WAVE - 1) / (CT / WAVE)));
  auto st = (hipStream_t)stream;
  if (wide) {
    hipLaunchKernelGGL(k_ctr_seg_adagrad<4>, grid, dim3(CT), 0, st, slab, keys_sorted, perm, grad,
                       scratch, n, D, plen, world, lg, lr, eps);
    if (chunks > 1)
      hipLaunchKernelGGL(k_ctr_seg_tail<4>, tail_grid, dim3(CT), 0, st, slab, keys_sorted,
                         scratch, n, D, plen, world, lg, lr, eps);
  } else {
    hipLaunchKernelGGL(k_ctr_seg_adagrad<1>, grid, dim3(CT), 0, st, slab, keys_sorted, perm, grad,
                       scratch, n, D, plen, world, lg, lr, eps);
    if (chunks > 1)
      hipLaunchKernelGGL(k_ctr_seg_tail<1>, tail_grid, dim3(CT), 0, st, slab, keys_sorted,
                         scratch, n, D, plen, world, lg, lr, eps);
  }
}

}  // namespace adapm
