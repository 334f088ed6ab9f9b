// App compute kernels (the reference's per-datapoint scalar loops become
// batched device kernels — SURVEY.md §2.5 inventory):
//   - KGE ComplEx score/grad + fused AdaGrad (reference
//     knowledge_graph_embeddings.cc:832-858 score/grad, 415-435 AdaGrad)
//   - word2vec SGNS step (reference word2vec.cc:679-745)
//   - MF NZSL+L2 update (reference apps/mf/update.h:32-69)
//
// Value layout convention (same as the reference apps): every key's value
// is [embedding(D) | adagrad_accum(D)], so AdaGrad state rides the same
// Push/Pull path. Kernels consume pulled rows and produce PUSH-ready
// additive deltas: [delta_emb(D) | grad^2(D)].
#pragma once
#include <cstddef>
#include <cstdint>

namespace adapm {

// The ComplEx and SGNS step kernels (classic and fused) hold a row's lanes
// in registers, at most 8 per thread of a 256-thread workgroup. ComplEx has
// D/2 lanes per row, SGNS D. Callers refuse longer rows before launching;
// the CPU twins have no such limit.
constexpr int STEP_MAX_LANES = 8 * 256;

// The fused CTR kernels (ctr_hip.hip) give a row's floats to the lanes of a
// lane group, 4 floats per lane where D % 4 == 0 and the pointers are 16-byte
// aligned, else 1. A group is at most one wave (64 lanes) and holds one
// column block of a row at a time; longer rows take further passes over the
// same keys. The limit below is 16 passes of the one-float mapping, 4 of the
// four-float one; the bindings refuse a longer row before enqueueing.
constexpr int CTR_MAX_DIM = 1024;

// Positions of the sorted key array that one lane group of ctr_update_fused
// sums serially (a "chunk").
constexpr int CTR_SEG_CHUNK = 32;

// ComplEx training step over B positives with N o-side negatives each.
//  s, r, o:   [B][2D]   pulled rows (emb | accum)
//  neg:       [B*N][2D] pulled negative-entity rows
//  ds,dr,do_,dneg: same shapes, outputs (push deltas)
//  loss:      [B] logistic loss of each positive (+ its negatives)
// D = embedding dim (even: first half real, second half imaginary).
void kge_complex_step_gpu(const float* s, const float* r, const float* o, const float* neg,
                          float* ds, float* dr, float* do_, float* dneg, float* loss,
                          int B, int N, int D, float lr, float eps, void* stream);
void kge_complex_step_cpu(const float* s, const float* r, const float* o, const float* neg,
                          float* ds, float* dr, float* do_, float* dneg, float* loss,
                          int B, int N, int D, float lr, float eps);

// ComplEx SIDES step: the reference's two-sided objective with L2 on the
// positive (reference knowledge_graph_embeddings.cc train(), ~:1106). One
// work item is a positive (s, r, o) with N object-side negatives (s, r, o'_j)
// and NS subject-side negatives (s'_j, r, o); each term is a logistic loss as
// in the step above and loss[b] sums the 1 + N + NS of them.
//  neg_o: [B*N][2D], neg_s: [B*NS][2D]; dneg_o, dneg_s likewise
// Each row occurrence gets ONE AdaGrad update of its summed gradient:
//  g_s = positive + N object-side terms + gamma_e * s
//  g_o = positive + NS subject-side terms + gamma_e * o
//  g_r = all 1 + N + NS terms + gamma_r * r
//  o'_j, s'_j: their own term, no regulariser (the reference regularises
//  positives only). The regulariser's value is not part of loss[b].
// With NS = 0 and both gammas 0 this is kge_complex_step, in its order of
// operations; the GPU launchers (classic and fused) then run the one-sided
// kernel itself, which is what makes the results the same bit for bit.
// Dropout is kge_complex_step_drop, further down.
void kge_complex_step_sides_gpu(const float* s, const float* r, const float* o,
                                const float* neg_o, const float* neg_s, float* ds, float* dr,
                                float* do_, float* dneg_o, float* dneg_s, float* loss, int B,
                                int N, int NS, int D, float lr, float eps, float gamma_e,
                                float gamma_r, void* stream);
void kge_complex_step_sides_cpu(const float* s, const float* r, const float* o,
                                const float* neg_o, const float* neg_s, float* ds, float* dr,
                                float* do_, float* dneg_o, float* dneg_s, float* loss, int B,
                                int N, int NS, int D, float lr, float eps, float gamma_e,
                                float gamma_r);

// Row tags for the fused slab-direct steps: which key occurrences of one
// batch share their slab row with another occurrence of the same batch.
// `tags` is a device array of one word per row; its contents before a step
// do not matter. Occurrence i is position i in the concatenation of up to
// four key arrays (counted together, whatever their role), and the total
// must stay below ROWTAG_SHARED. Three launches on one stream, then the step:
//   tag   every occurrence i stores tags[row] = i; where several name one
//         row, any one of them wins;
//   flag  every occurrence i loads tags[row] and stores ROWTAG_SHARED there
//         unless it finds its own i;
//   bits  every occurrence rewrites the whole word of its row in `bits`, one
//         bit per row, from the 32 tags that word stands for.
// After tag and flag, tags[row] == ROWTAG_SHARED exactly for the rows that
// two or more occurrences name: a row named once keeps its i; of a row named
// more than once all occurrences but the winner read the winner's index or
// ROWTAG_SHARED, never their own, and store ROWTAG_SHARED. The step reads
// bit `row` of `bits`, a bitmap small enough to stay in cache (the tags are
// not: a step kernel that read them gave back all that the passes saved,
// profiles/kge_rowtags_stats.txt). The
// tag pass writes every tag, and the bits pass every bitmap word, that the
// step goes on to ask about, so nothing is cleaned up afterwards and no
// launch holds a read-modify-write: racing stores to one word all lead to
// the same final state, and the kernel boundaries order the passes and the
// step. Tags and bits of rows outside the batch are stale and never read.
// Keys must be row indices (single-rank identity layout: row == key) below
// `rows`; `tags` holds 32 * rowtag_words(rows) words, 128-byte aligned, and
// `bits` rowtag_words(rows).
constexpr uint32_t ROWTAG_SHARED = 0xFFFFFFFFu;
struct RowTagKeys {
  const int64_t* keys[4];  // DEVICE pointers
  int64_t n[4];
  int count;  // arrays in use
};
inline int64_t rowtag_words(int64_t rows) { return (rows + 31) / 32; }
void rowtag_tag_gpu(uint32_t* tags, const RowTagKeys& ks, void* stream);  // tests only
void rowtag_flag_gpu(uint32_t* tags, const RowTagKeys& ks, void* stream);
void rowtag_bits_gpu(const uint32_t* tags, uint32_t* bits, const RowTagKeys& ks, void* stream);

// The tag pass of a step whose first n_copy keys still sit in pinned,
// device-visible host memory: occurrence i < n_copy reads src_host[i],
// writes it to dst[i] (device) and tags its row; occurrence n_copy + j,
// j < n_dev, tags the row of dev_keys[j] (device keys, e.g. drawn
// negatives). One launch on `stream` in place of copy_keys_gpu plus a tag
// pass. Returns false, with nothing enqueued, if src_host is not
// device-visible.
bool keys_land_gpu(uint32_t* tags, int64_t* dst, const int64_t* src_host, int64_t n_copy,
                   const int64_t* dev_keys, int64_t n_dev, void* stream);

// FUSED ComplEx step: reads entity/relation rows DIRECTLY from the slab
// and accumulates the AdaGrad-transformed deltas back — no intermediate
// pull/push buffers (the classic path pays a gather write + kernel read +
// delta write + scatter read; this saves all four). keys_* are DEVICE
// int64 pointers.
// Writes: with `bits` (the row tags' bitmap after the three passes over
// exactly these keys, world == 1 only) plain stores on rows unique in the
// batch, atomic adds on shared ones — a float atomic costs ~4-5x the plain
// store of the same bytes and only a shared row needs it. The caller
// guarantees that nothing else writes the slab while the launch runs.
// Without bits every write is atomic. Either way duplicate keys within the
// batch see hogwild-style concurrent updates (async-PS semantics).
// shared_stat (optional, with bits) accumulates the number of occurrences
// that took the atomic path.
// Addressing modes (row_at): world >= 1 — identity layout, key k at
// (k/world)*plen (single-rank fast path, zero host work); world == 0 —
// keys_* carry precomputed float OFFSETS into the slab (the world>1 /
// relocated-layout path: the host pass resolves offsets and compacts
// all-local samples, remote ones take the classic path).
void kge_complex_step_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                const int64_t* keys_o, const int64_t* keys_neg, float* loss,
                                int B, int N, int D, int32_t plen, int world, float lr,
                                float eps, void* stream, const uint32_t* bits = nullptr,
                                unsigned long long* shared_stat = nullptr);

// FUSED sides step: kge_complex_step_sides on the slab's own rows, with the
// addressing modes, the `bits` contract and shared_stat of
// kge_complex_step_fused_gpu. The tags must cover all five key arrays.
void kge_complex_step_sides_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                      const int64_t* keys_o, const int64_t* keys_neg_o,
                                      const int64_t* keys_neg_s, float* loss, int B, int N,
                                      int NS, int D, int32_t plen, int world, float lr,
                                      float eps, float gamma_e, float gamma_r, void* stream,
                                      const uint32_t* bits = nullptr,
                                      unsigned long long* shared_stat = nullptr);
void kge_complex_step_sides_fused_offs_cpu(float* slab, const int64_t* offs_s,
                                           const int64_t* offs_r, const int64_t* offs_o,
                                           const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                           float* loss, int B, int N, int NS, int D, float lr,
                                           float eps, float gamma_e, float gamma_r);

// ComplEx sides step WITH DROPOUT (kge_drop_hip.hip; reference do_dropout in
// train(), --dropout_entity / --dropout_relation). One sample is the sides
// step's: a positive (s, r, o), N object-side negatives (s, r, o'_j), NS
// subject-side negatives (s'_j, r, o). Its scored triples are numbered
//   t = 0             the positive
//   t = 1 .. N        the object-side negatives
//   t = N+1 .. N+NS   the subject-side negatives,        T = 1 + N + NS
// and every scored triple draws fresh masks for each of its three rows, over
// the D embedding floats (real and imaginary halves independently), never
// over the accumulators:
//   psi_t = psi(m_s,t * s_t, m_r,t * r, m_o,t * o_t),  mask values 0 or scale.
// loss[b] sums the same 1 + N + NS logistic terms (softplus1pf on the GPU).
// The gradient is the true gradient of that loss: a dropped component gets no
// score gradient from that triple (an exact 0), a kept one `scale` times the
// gradient with respect to the masked value. gamma_e and gamma_r act on the
// STORED rows of the positive and every row occurrence gets ONE AdaGrad update
// of its summed gradient, exactly as in the sides step.
// Mask. For complex lane k < dc = D/2 of triple t of sample b (b = position in
// THIS call's arrays; on the general path, in the compacted ones), in 64 bits:
//   idx = (b * T + t) * dc + k
//   h   = pcg_hash64(drop_seed ^ idx * 0x9e3779b97f4a7c15)   (as alias_draw)
// Field f = bits [10f, 10f + 10) of h, f = 0..5 = (s_re, s_im, r_re, r_im,
// o_re, o_im), where s / o name the ROLE in the scored triple (s'_j takes the
// s fields, o'_j the o fields). A component is kept iff its field >= thr:
//   thr_e = lround(p_e * 1024) for the s and o fields, thr_r likewise from p_r,
//   both in [0, 1023] (drop_threshold; the bindings check);
//   scale = 1024 / (1024 - thr) rounded to fp32 (drop_scale), the reciprocal
//   of the keep probability actually realised.
// One hash per complex lane per triple yields all six masks; nothing about a
// mask is stored. With thr_e == thr_r == 0 the entry points run the sides
// entry points themselves (bit-equal results, docs/PARITY.md 2.5). The fused
// step has the addressing modes, the `bits` contract (tags over all five key
// arrays) and shared_stat of kge_complex_step_sides_fused_gpu. The CPU twins
// are serial; the fused one works in place in the fused kernel's order.
// Unlike the reference, the gradient is chained through the mask and the
// regulariser sees the stored values (docs/PARITY.md 2.3).
constexpr int DROP_FIELD_BITS = 10;
constexpr int DROP_ONE = 1 << DROP_FIELD_BITS;  // 1024
int drop_threshold(double p);  // lround(p * 1024), or -1 if that is not in [0, 1023]
inline float drop_scale(int thr) { return (float)((double)DROP_ONE / (DROP_ONE - thr)); }
void kge_complex_step_drop_gpu(const float* s, const float* r, const float* o,
                               const float* neg_o, const float* neg_s, float* ds, float* dr,
                               float* do_, float* dneg_o, float* dneg_s, float* loss, int B,
                               int N, int NS, int D, float lr, float eps, float gamma_e,
                               float gamma_r, int thr_e, int thr_r, uint64_t drop_seed,
                               void* stream);
void kge_complex_step_drop_cpu(const float* s, const float* r, const float* o,
                               const float* neg_o, const float* neg_s, float* ds, float* dr,
                               float* do_, float* dneg_o, float* dneg_s, float* loss, int B,
                               int N, int NS, int D, float lr, float eps, float gamma_e,
                               float gamma_r, int thr_e, int thr_r, uint64_t drop_seed);
void kge_complex_step_drop_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                     const int64_t* keys_o, const int64_t* keys_neg_o,
                                     const int64_t* keys_neg_s, float* loss, int B, int N, int NS,
                                     int D, int32_t plen, int world, float lr, float eps,
                                     float gamma_e, float gamma_r, int thr_e, int thr_r,
                                     uint64_t drop_seed, void* stream,
                                     const uint32_t* bits = nullptr,
                                     unsigned long long* shared_stat = nullptr);
void kge_complex_step_drop_fused_offs_cpu(float* slab, const int64_t* offs_s,
                                          const int64_t* offs_r, const int64_t* offs_o,
                                          const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                          float* loss, int B, int N, int NS, int D, float lr,
                                          float eps, float gamma_e, float gamma_r, int thr_e,
                                          int thr_r, uint64_t drop_seed);

// ComplEx step with CHUNK-SHARED negatives (kge_chunk_hip.hip). The batch of B
// positives (s_b, r_b, o_b) is cut into chunks of C >= 1: n_chunks =
// ceil(B / C), chunk c holds the positives [cC, min(B, (c+1)C)), so the last
// chunk may be short. The negatives are n_chunks * M entity occurrences; chunk
// c owns neg[cM .. cM + M) and every positive of the chunk is scored against
// all M of them (the objective of PyTorch-BigGraph and DGL-KE; beyond the
// reference, whose train() draws negatives per positive). Object side only,
// no regulariser, no dropout. With c(b) = b / C:
//   loss[b] = softplus(-psi(s_b, r_b, o_b)) + sum_{j<M} softplus(psi(s_b, r_b, n_{c(b),j}))
// (softplus1pf on the GPU). With u_b = s_b * r_b as the real vector
// [u_re | u_im], psi(s_b, r_b, x) = u_b . x, and
//   g0_b = -sigmoid(-psi0_b),  G[b][j] = sigmoid(psi[b][j])
//   a_b  = g0_b o_b + sum_j G[b][j] n_j         gradient w.r.t. u_b  (G N)
//   g_s  = a_b * conj(r_b),  g_r = a_b * conj(s_b)   component-wise, as k_kge_step
//   g_o  = g0_b u_b
//   g_{n_j} = sum_{b in chunk} G[b][j] u_b      (G^T U)
// Every row OCCURRENCE gets ONE AdaGrad update (adagrad_delta, accumulator +=
// g^2) computed from the pre-step row: s, r and o one per positive, a negative
// occurrence one update of its gradient summed over the chunk's positives (the
// rule of R in the grouped RESCAL step). A key that occurs twice (twice in one
// chunk, in two chunks, or as a negative and as some positive's s or o) is two
// occurrences; on the slab they land hogwild, as for every fused step. With
// C = 1 this is kge_complex_step with N = M.
//  s, r, o, ds, dr, do_ [B][2D]; neg, dneg [n_chunks * M][2D]; loss [B]
//  scratch: kge_chunk_scratch_floats(B, M) floats on the device, contents
//  irrelevant (G [B][M], g0 [B], the loss shares [B][4])
// Two launches on `stream` (scores, then update over (chunk, column block));
// no atomic touches a partial sum, and a row unique in the batch is written
// with plain stores when `bits` is given, so on unique keys the result does
// not depend on scheduling. 1 <= C <= KGE_CHUNK_MAX_C, 1 <= M <=
// KGE_CHUNK_MAX_M; the GPU entries need D % 8 == 0 (both halves of a row
// 16-byte aligned, a K-chunk of 4 never straddles re and im) and loop over D,
// so STEP_MAX_LANES does not bound it; the CPU twin takes any even D. Callers
// check all of it. B < 1 is a no-op. The fused entry has the addressing modes
// (row_at) and the `bits` contract of kge_complex_step_fused_gpu, the tags
// covering s | r | o | neg.
constexpr int KGE_CHUNK_MAX_C = 64;
constexpr int KGE_CHUNK_MAX_M = 256;
inline int64_t kge_chunk_scratch_floats(int64_t B, int64_t M) { return B * (M + 5); }
// dynamic LDS of the update launch (150,528 B at the limits, of 163,840 B)
size_t kge_chunk_update_lds_bytes(int C, int M);
void kge_complex_step_chunk_gpu(const float* s, const float* r, const float* o, const float* neg,
                                float* ds, float* dr, float* do_, float* dneg, float* loss,
                                float* scratch, int B, int C, int M, int D, float lr, float eps,
                                void* stream);
void kge_complex_step_chunk_cpu(const float* s, const float* r, const float* o, const float* neg,
                                float* ds, float* dr, float* do_, float* dneg, float* loss, int B,
                                int C, int M, int D, float lr, float eps);
void kge_complex_step_chunk_fused_gpu(float* slab, const int64_t* keys_s, const int64_t* keys_r,
                                      const int64_t* keys_o, const int64_t* keys_neg, float* loss,
                                      float* scratch, int B, int C, int M, int D, int32_t plen,
                                      int world, float lr, float eps, void* stream,
                                      const uint32_t* bits = nullptr);

// CPU tier of the offsets-mode fused steps (exercises the world>1 fused
// protocol path in the gloo multi-process tests; serial, in-place).
void kge_complex_step_fused_offs_cpu(float* slab, const int64_t* offs_s, const int64_t* offs_r,
                                     const int64_t* offs_o, const int64_t* offs_neg, float* loss,
                                     int B, int N, int D, float lr, float eps);
void w2v_sgns_step_fused_offs_cpu(float* slab, const int64_t* offs_ctr, const int64_t* offs_ctx,
                                  const int64_t* offs_neg, float* loss, int B, int N, int D,
                                  float lr, float eps);
void mf_update_step_fused_offs_cpu(float* slab, const int64_t* offs_w, const int64_t* offs_h,
                                   const float* x, float* loss, int B, int R, float lr,
                                   float lambda, float eps);

// FUSED SGNS step: slab-direct reads + AdaGrad writes, same addressing
// modes as kge_complex_step_fused_gpu. Every write is atomic: the kernel
// takes no row tags. It writes through the same per-lane helper as the
// ComplEx step (slab_adagrad in kernels_hip.hip) with shared = true, so
// adopting the tags means passing the row's bit there instead.
void w2v_sgns_step_fused_gpu(float* slab, const int64_t* keys_ctr, const int64_t* keys_ctx,
                             const int64_t* keys_neg, float* loss, int B, int N, int D,
                             int32_t plen, int world, float lr, float eps, void* stream);

// FUSED MF step (slab-direct NZSL+L2; same contract as above).
void mf_update_step_fused_gpu(float* slab, const int64_t* keys_w, const int64_t* keys_h,
                              const float* x, float* loss, int B, int R, int32_t plen,
                              int world, float lr, float lambda, float eps, void* stream);

// FUSED CTR embedding step (identity layout only: key k at (k/world)*plen),
// the two halves of a wide-and-deep step on either side of the dense tower.
//
// ctr_gather_fused_gpu: x[i][0:D] = emb half of the row of keys[i], for the
// n key occurrences of a batch in the caller's order. No unique, no
// accumulator half, no intermediate buffer.
//
// ctr_update_fused_gpu: for every distinct key u of the batch
//   g = sum of grad[i] over the occurrences i of u
//   emb += -lr * g / sqrt(acc + g*g + eps),  acc += g*g
// written into the row in place: ONE AdaGrad update of the complete sum per
// key, as the classic step does after its unique + scatter-add. Inputs:
//   keys_sorted [n]  the batch's keys, ascending (device)
//   perm [n]         occurrence of each sorted position: keys_sorted[p] is
//                    the key of occurrence perm[p], grad row perm[p]
//   grad [n][D]      gradient of x
//   scratch          2 * D * ceil(n / CTR_SEG_CHUNK) floats, contents irrelevant
// How the work is split: the sorted array is cut into chunks of CTR_SEG_CHUNK
// positions and every chunk goes to one lane group (the row's column block
// spread over 1..64 lanes, so a wave carries 64 / lanes chunks), whatever the
// key distribution. A group walks its chunk with the sum of the current run
// of equal keys in registers. Everything it needs to know about a run it
// reads from keys_sorted: a run begins inside the chunk if the position
// before it holds another key (or is the array's start) and ends inside if
// the position after it does (or is the array's end).
//   - a run that begins and ends inside is a whole segment: the group reads
//     the row, applies AdaGrad and stores both halves;
//   - a run open on the left (whether or not it is open on the right too)
//     stores its sum to scratch[chunk][0], one open only on the right to
//     scratch[chunk][1].
// A second launch gives one wave to every chunk whose slot 1 is in use (the
// HEAD of a segment that spans chunks; exactly one per such segment, since
// every later chunk of the segment sees it open on the left). The wave finds
// the segment's end by binary search in keys_sorted, so it knows the chunks
// whose slot 0 belongs to the segment; its groups add them in a fixed strided
// order, a butterfly over the groups joins their sums, and group 0 does the
// AdaGrad write. A group serially adds at most CTR_SEG_CHUNK gradient rows,
// or the partials of one segment.
// Every slab write is a plain store and no launch holds an atomic: each
// distinct key is written by exactly one group. The order of all additions
// is fixed by (n, D, keys), so two runs from one state agree bit for bit.
// The caller guarantees what plain stores need: nothing else writes the slab
// while the launches run, i.e. the server has a single worker thread and
// every slab writer is enqueued on `stream`. 1 <= D <= CTR_MAX_DIM; n == 0
// is a no-op.
void ctr_gather_fused_gpu(const float* slab, const int64_t* keys, float* x, int64_t n, int D,
                          int32_t plen, int world, void* stream);
void ctr_update_fused_gpu(float* slab, const int64_t* keys_sorted, const int64_t* perm,
                          const float* grad, float* scratch, int64_t n, int D, int32_t plen,
                          int world, float lr, float eps, void* stream);

// ComplEx scoring only (evaluation): score[b][e] = psi(s_b, r_b, cand_e)
//  cand: [E][2D] candidate entity rows; scores: [B][E]
void kge_complex_score_gpu(const float* s, const float* r, const float* cand, float* scores,
                           int B, int E, int D, void* stream);
void kge_complex_score_cpu(const float* s, const float* r, const float* cand, float* scores,
                           int B, int E, int D);

// RESCAL training step (reference knowledge_graph_embeddings.cc:895-922):
// score = e_s^T R e_o, R is D x D. Entity rows [emb(D) | accum(D)],
// relation rows [R(D*D) | accum(D*D)]. Math uses the factorization
// u = R^T e_s (once), w = sum_o c_o e_o, de_s = R w, dR = e_s w^T — so a
// triple with N negatives costs ~3 D^2 + N D instead of N D^2.
void rescal_step_gpu(const float* s, const float* r, const float* o, const float* neg,
                     float* ds, float* drl, float* do_, float* dneg, float* loss, int B, int N,
                     int D, float lr, float eps, void* stream);
void rescal_step_cpu(const float* s, const float* r, const float* o, const float* neg,
                     float* ds, float* drl, float* do_, float* dneg, float* loss, int B, int N,
                     int D, float lr, float eps);

// RESCAL SIDES step: the two-sided objective of the ComplEx sides step above
// (the reference trains both scorers with one train()) for psi = s^T R o. One
// work item is a positive (s, R, o) with N object-side negatives o'_j and NS
// subject-side negatives s'_j; loss[b] sums the 1 + N + NS logistic terms and
// leaves the regulariser's value out.
//  neg_o: [B*N][2D], neg_s: [B*NS][2D]; dneg_o, dneg_s likewise
// Factorisation, with u = R^T s and v = R o:
//  object pass   c_0 = -sigmoid(-psi_0), c_j = sigmoid(psi_j), psi_j = u . o_j
//                w = c_0 o + sum_j c_j o'_j          grad o'_j = c_j u
//  subject pass  a_j = sigmoid(s'_j . v)
//                z = sum_j a_j s'_j                  grad s'_j = a_j v
//  positive      grad s = R w + gamma_e s
//                grad o = c_0 u + R^T z + gamma_e o
//                grad R = s w^T + z o^T + gamma_r R
// so a sample costs ~6 D^2 + (N + NS) D. Each row occurrence gets ONE AdaGrad
// update of its summed gradient; o is written after the subject pass. D <= 196
// on the GPU (R and six D-vectors in LDS); callers check it. The bindings run
// rescal_step itself when NS = 0 and both gammas are 0.
void rescal_step_sides_gpu(const float* s, const float* r, const float* o, const float* neg_o,
                           const float* neg_s, float* ds, float* drl, float* do_,
                           float* dneg_o, float* dneg_s, float* loss, int B, int N, int NS,
                           int D, float lr, float eps, float gamma_e, float gamma_r,
                           void* stream);
void rescal_step_sides_cpu(const float* s, const float* r, const float* o, const float* neg_o,
                           const float* neg_s, float* ds, float* drl, float* do_,
                           float* dneg_o, float* dneg_s, float* loss, int B, int N, int NS,
                           int D, float lr, float eps, float gamma_e, float gamma_r);

// FUSED RESCAL step (rescal_fused_hip.hip): the one-sided grouped step (N
// object-side negatives, no regulariser) on the slab's own rows, offsets mode
// only: every row is slab + offs[i], offs in floats and multiples of 4 (rows
// start on 16-byte boundaries; the binding checks it). Entity rows are
// [emb(D) | acc(D)], relation rows [R(D*D) | acc(D*D)], R row-major.
//   offs_s, offs_o [B], offs_neg [B*N]   the triples, SORTED BY RELATION
//   offs_rg [G], starts [G+1]            group g = triples [starts[g],
//                                        starts[g+1]), all of relation offs_rg[g];
//                                        no group is empty
//   tiles [n_tiles][2]                   (g, m0) for every 16-row tile of every
//                                        group, m0 counted within the group
//   U, W, Sc [B][D]                      scratch, contents irrelevant
//   loss [B]                             in the sorted order
// Four launches on `stream`:
//   1  U = S_g R_g (u_b = R^T s_b), s gathered from the slab; Sc[b] = s_b
//   2  per triple: psi_j = u . o_j, c_j = -y_j / (1 + exp(y_j psi_j)),
//      W[b] = sum_j c_j o_j; o and every o'_j get their AdaGrad update of
//      c_j u in place; loss[b]
//   3  s_b += AdaGrad(R_g W[b])           from the accumulators, no ds buffer
//   4  R_g += AdaGrad(sum_b Sc[b] W[b]^T) the group-summed gradient, as
//      rescal_step_grouped
// Launch 3 reads the R that launch 4 writes, and launch 4 reads Sc, not the s
// that launch 3 has moved: on a batch of distinct keys the result is the
// grouped step's. Every slab write is an atomicAdd of the delta and of g^2,
// the accumulator read before it a plain load, as slab_adagrad(shared = true):
// a key named more than once in a batch sees hogwild-style concurrent updates
// (async-PS semantics), and an entity that is an o or o' and also an s has had
// its accumulator moved by launch 2 when launch 3 reads it. That is the
// contract of every fused step here.
// D % 4 == 0, 4 <= D <= RESCAL_FUSED_MAX_DIM; callers check. B, G or n_tiles
// < 1 is a no-op. adagrad_delta and the softplus are repeated in the .hip
// file rather than shared with kernels_hip.hip, whose KPT = 8 kernels have a
// register allocation that moving code around has broken before.
// The CPU twin is serial and in place: per triple it takes a copy of s, runs
// launch 2's loop on the rows themselves, then updates s; R is updated at the
// end of its group.
constexpr int RESCAL_FUSED_MAX_DIM = 256;
void rescal_step_fused_gpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                           const int64_t* offs_neg, const int64_t* offs_rg, const int32_t* starts,
                           const int32_t* tiles, int n_tiles, float* U, float* W, float* Sc,
                           float* loss, int B, int G, int N, int D, float lr, float eps,
                           void* stream);
void rescal_step_fused_offs_cpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                                const int64_t* offs_neg, const int64_t* offs_rg,
                                const int32_t* starts, float* loss, int B, int G, int N, int D,
                                float lr, float eps);

// FUSED RESCAL SIDES step (rescal_fused_hip.hip): the two-sided objective of
// rescal_step_sides above (N object-side negatives o'_j, NS subject-side
// negatives s'_j, gamma_e on the positive's s and o, gamma_r on its R) on the
// slab's own rows, with the layout, the arguments and the limits of
// rescal_step_fused_gpu and the result of rescal_step_sides_grouped: every row
// occurrence gets ONE AdaGrad update of its summed gradient, dR is the AdaGrad
// transform of the group-summed gradient, each of a group's Bg positives
// adding gamma_r R, and loss[b] sums the 1 + N + NS logistic terms without
// the regulariser.
//   offs_neg_o [B*N], offs_neg_s [B*NS]  the negatives, in the sorted order
//   scratch                              6*B*D + B floats, contents irrelevant:
//                                        U, V, W, Z, Sc, Oc [B][D], then c0 [B]
// Four launches on `stream`, with u_b = R^T s_b and v_b = R o_b:
//   1  U = S_g R_g and V = O_g R_g^T over 2 * n_tiles workgroups, s and o
//      gathered from the slab; Sc[b] = s_b, Oc[b] = o_b
//   2  per triple, object pass: psi_j = u . o_j, c_j as in the one-sided step,
//      W[b] = c_0 o + sum_j c_j o'_j, every o'_j updated in place with c_j u,
//      the positive o scored but NOT written; subject pass: a_j =
//      sigmoid(v . s'_j), Z[b] = sum_j a_j s'_j, every s'_j updated in place
//      with a_j v; c0[b], loss[b]
//   3  s_b += AdaGrad(R_g W[b] + gamma_e Sc[b]) and
//      o_b += AdaGrad(c0[b] U[b] + R_g^T Z[b] + gamma_e Oc[b]) over 2 * n_tiles
//      workgroups, from the accumulators
//   4  R_g += AdaGrad(sum_b (Sc[b] W[b]^T + Z[b] Oc[b]^T) + gamma_r Bg R_g),
//      one product over the concatenated K = 2 Bg; R is read with a plain
//      load before the atomics
// Launch 3 reads the R that launch 4 writes, and launch 4 reads the snapshots
// Sc and Oc, never the rows launch 3 has moved. Slab writes follow the fused
// steps' contract given above rescal_step_fused_gpu: atomicAdd of the delta and
// of g^2, the accumulator read before it with a plain load, hogwild updates
// for a key named more than once. The loss is summed with softplus1pf, as in
// every sides kernel (docs/PARITY.md, 2.5). The binding runs
// rescal_step_fused_gpu / _offs_cpu itself when NS = 0 and both gammas are 0.
// The CPU twin is serial and in place: per triple it takes copies of s and o,
// runs both passes on the rows themselves, then updates s and o; R is updated
// at the end of its group.
void rescal_step_sides_fused_gpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                                 const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                 const int64_t* offs_rg, const int32_t* starts,
                                 const int32_t* tiles, int n_tiles, float* scratch, float* loss,
                                 int B, int G, int N, int NS, int D, float lr, float eps,
                                 float gamma_e, float gamma_r, void* stream);
void rescal_step_sides_fused_offs_cpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                                      const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                      const int64_t* offs_rg, const int32_t* starts, float* loss,
                                      int B, int G, int N, int NS, int D, float lr, float eps,
                                      float gamma_e, float gamma_r);

// RESCAL sides step WITH DROPOUT (rescal_drop_hip.hip; reference do_dropout in
// train(), which both scorers share). One sample is the sides step's: a
// positive (s, R, o), N object-side negatives (s, R, o'_j), NS subject-side
// negatives (s'_j, R, o). Its scored triples are numbered
//   t = 0             the positive
//   t = 1 .. N        the object-side negatives
//   t = N+1 .. N+NS   the subject-side negatives,        T = 1 + N + NS
// and every scored triple draws fresh masks for its three rows, over the
// embedding floats (D of an entity row, D*D of R), never over the accumulators:
//   psi_t = (m_s ⊙ s_t)^T (M_t ⊙ R) (m_o ⊙ o_t),  mask values 0 or scale,
// with drop_threshold, drop_scale and the 10-bit fields of the ComplEx drop
// step above: thr_e = lround(p_e * 1024) for the entity masks, thr_r likewise
// from p_r, a component kept iff its field >= thr, scale = 1024 / (1024 - thr).
// Objective and gradient (the choices docs/PARITY.md 2.3 records for ComplEx):
//   - psi is taken on the masked rows; loss[b] sums the T logistic terms
//     (softplus1pf on the GPU) and leaves the regulariser's value out;
//   - the gradient is the true gradient through the masks: a dropped
//     component gets an exact 0 from that triple, a kept one `scale` times the
//     gradient with respect to the masked value;
//   - gamma_e and gamma_r act on the STORED rows of the positive;
//   - every entity row occurrence gets ONE AdaGrad update of its summed
//     gradient (s: t = 0..N, o: t = 0 and t > N, o'_j and s'_j their own term);
//   - R gets the AdaGrad transform of the group-summed gradient plus
//     gamma_r * Bg * R, as in rescal_step_sides_grouped. With groups of one
//     positive (starts = 0..B) that is the per-triple semantics.
// The gradient of R is sum_t g_t * M_t ⊙ (s~_t o~_t^T): with a fresh M_t per
// triple nothing factors through u = R^T s or v = R o, so a triple costs about
// 3 D^2 whatever one does.
// Mask index, everything in 64 bits: q = b * T + t, b the position in THIS
// call's arrays (the sorted order; on the general path the sorted and
// compacted one).
//   entity masks    for k < D: h = pcg_hash64(drop_seed ^ (q*D + k) * 0x9e3779b97f4a7c15)
//                   field 0 (bits 0..9) is the subject ROLE of the triple (s or
//                   s'_j), field 1 (bits 10..19) the object role (o or o'_j);
//                   kept iff field >= thr_e
//   relation masks  element e = i*D + j of R (row-major, psi = sum s_i R_ij o_j),
//                   Q = (D*D + 3) / 4:
//                   h = pcg_hash64(~drop_seed ^ (q*Q + (e >> 2)) * 0x9e3779b97f4a7c15)
//                   field e & 3, kept iff field >= thr_r: one hash serves four
//                   consecutive floats of R, one 16-byte load
// With thr_r == 0 no relation hash is taken (every element kept, scale 1), and
// likewise thr_e and the entity hash. The entry points do NOT special-case
// thr_e == thr_r == 0: the drop kernels then run with every component kept, and
// the result is within tolerance of the sides step, not bit-equal to it.
//
// Layout: samples sorted by relation, group g = samples [starts[g],
// starts[g+1]), no group empty; tiles [n_tiles][2] = (g, m0) for every run of
// 16 samples of every group, as for rescal_step_fused_gpu. Two launches:
//   1  one workgroup per tile: R_g staged in LDS once, then the tile's
//      positives and their T triples one after the other. Entity rows are
//      finished here. The tile's share of dR is summed in registers across
//      all its triples and stored once, to scratch[tile][D*D].
//   2  per group: the tile partials added in tile order, plus gamma_r*Bg*R,
//      then R's AdaGrad update.
// No atomic touches a partial, so on distinct keys the step is bit-reproducible.
// The classic variant reads pulled rows ([n][2D], rm [G][2 D*D]) and writes
// push deltas of the same shapes, any 1 <= D <= RESCAL_DROP_MAX_DIM. The fused
// variant works on slab + offs[i] with the fused steps' contract given above
// rescal_step_fused_gpu (atomicAdd of the delta and of g^2, the accumulator
// read before it with a plain load; R updated by launch 2) and also needs
// D % 4 == 0. starts and tiles are DEVICE pointers for the GPU entries, starts
// a host pointer for the CPU twins; scratch holds n_tiles * D*D floats,
// contents irrelevant. RESCAL_DROP_MAX_DIM is what R, nine D-vectors and the
// register-held dR share of a workgroup fit (160 KB of LDS, no scratch memory);
// callers check it. The CPU twins are serial; the fused one works in place in
// the manner of rescal_step_sides_fused_offs_cpu (copies of s and o, the
// negatives updated as they are scored, R at the end of its group).
constexpr int RESCAL_DROP_MAX_DIM = 196;
void rescal_step_drop_gpu(const float* s, const float* rm, const float* o, const float* neg_o,
                          const float* neg_s, float* ds, float* drl, float* do_, float* dneg_o,
                          float* dneg_s, const int32_t* starts, const int32_t* tiles, int n_tiles,
                          float* scratch, float* loss, int B, int G, int N, int NS, int D,
                          float lr, float eps, float gamma_e, float gamma_r, int thr_e, int thr_r,
                          uint64_t drop_seed, void* stream);
void rescal_step_drop_cpu(const float* s, const float* rm, const float* o, const float* neg_o,
                          const float* neg_s, float* ds, float* drl, float* do_, float* dneg_o,
                          float* dneg_s, const int32_t* starts, float* loss, int B, int G, int N,
                          int NS, int D, float lr, float eps, float gamma_e, float gamma_r,
                          int thr_e, int thr_r, uint64_t drop_seed);
void rescal_step_drop_fused_gpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                                const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                const int64_t* offs_rg, const int32_t* starts,
                                const int32_t* tiles, int n_tiles, float* scratch, float* loss,
                                int B, int G, int N, int NS, int D, float lr, float eps,
                                float gamma_e, float gamma_r, int thr_e, int thr_r,
                                uint64_t drop_seed, void* stream);
void rescal_step_drop_fused_offs_cpu(float* slab, const int64_t* offs_s, const int64_t* offs_o,
                                     const int64_t* offs_neg_o, const int64_t* offs_neg_s,
                                     const int64_t* offs_rg, const int32_t* starts, float* loss,
                                     int B, int G, int N, int NS, int D, float lr, float eps,
                                     float gamma_e, float gamma_r, int thr_e, int thr_r,
                                     uint64_t drop_seed);

// word2vec SGNS step: per center/context pair with N negatives.
//  ctr:  [B][2D] center (syn0) rows;  ctx: [B][2D] context (syn1) rows
//  neg:  [B*N][2D] negative (syn1) rows
//  outputs: push deltas, same shapes; loss [B]
void w2v_sgns_step_gpu(const float* ctr, const float* ctx, const float* neg, float* dctr,
                       float* dctx, float* dneg, float* loss, int B, int N, int D, float lr,
                       float eps, void* stream);
void w2v_sgns_step_cpu(const float* ctr, const float* ctx, const float* neg, float* dctr,
                       float* dctx, float* dneg, float* loss, int B, int N, int D, float lr,
                       float eps);

// word2vec WINDOW step (w2v_window_hip.hip; reference word2vec.cc:679-745, one
// context window per sentence position): a token stream goes in, and the
// subsampling, the windows, the pairs and the negatives are made where they
// are used.
//
// Inputs of one call (W2VWindowArgs)
//   tok[T]       int32 word ids in [0, V), in corpus order
//   starts[S+1]  int32, non-decreasing, starts[0] = 0, starts[S] = T; sentence
//                s is [starts[s], starts[s+1]), empty sentences allowed
//   keep[V]      float keep probabilities, or null for none
//   prob[n], alias[n]  the unigram alias table of sampling.py, n <= V
//   W >= 1, 0 <= N <= 63, a 64-bit seed
// GOLD = 0x9e3779b97f4a7c15 and sd[k] = pcg_hash64(seed + k), k = 0, 1, 2, in
// wrapping 64-bit arithmetic; pcg_hash64 is alias_draw's.
//
// Rules
//  1 Subsample. Position p is kept iff u < keep[tok[p]], with
//    h = pcg_hash64(sd[0] ^ p*GOLD) and u = float((h >> 40) & 0xffffff) * 2^-24
//    (the bits alias_draw uses for its u). A null keep keeps everything.
//  2 Compact. Kept tokens keep their order; c is a token's index among the
//    kept ones, ctok[c] its word, a sentence is its kept tokens, n_kept their
//    number.
//  3 Window. For centre c, b = 1 + pcg_hash64(sd[1] ^ c*GOLD) % W.
//  4 Pairs. For a = W-b .. W+b, a != W, ascending, j = c - W + a; if j lies in
//    c's compacted sentence, (ctr = ctok[c], ctx = ctok[j]) is a pair.
//  5 Negatives. Draw d < N of that pair is alias_draw's rule (slot = h % n,
//    u from bits 40..63, word = u < prob[slot] ? slot : alias[slot]) on
//    h = pcg_hash64(sd[2] ^ ((c*(2W+1) + a)*N + d) * GOLD). A draw equal to the
//    centre is not skipped (the pair steps do not skip it either).
//  6 Rows. The centre row has key 2*ctr (syn0), a target row key 2*w + 1
//    (syn1). Identity layout, one rank: key k is row k of the slab, rows are
//    [emb(D) | acc(D)] and `plen` floats apart.
//  7 Step of a centre. Its row is read once. For each of its pairs in order,
//    and for target t = 0 (ctx, y = +1), then t = 1..N (y = -1):
//      dot = c_emb . x_emb,  g = -y * sigmoid(-y * dot)
//      the target gets one AdaGrad update of g * c_emb, written as atomics
//      (delta and g^2, the accumulator read with a plain load before them)
//      a_c += g * x_emb
//  8 Centre update. After a pair's 1 + N targets the centre gets one AdaGrad
//    update of a_c, applied to the held copy (emb and acc both); the next
//    pair scores against it, as the reference's per-pair syn0 update does.
//    After the last pair `held - read` of both halves is added to the slab
//    with atomics. A centre without pairs writes nothing.
//  9 Outputs. loss[c] sums the softplus terms of all of c's pairs (log(1 +
//    exp(-y dot)), the sides kernels' softplus1pf on the GPU), loss[c] = 0 for
//    n_kept <= c < T; counts[0] = n_kept, counts[1] = number of pairs, both
//    on the device. Nothing comes back to the host; no entry synchronises.
//
// Hogwild contract, as for every fused step: rows named by several centres
// see concurrent updates (in a window that is every syn1 row of a sentence
// longer than two). Within a centre the GPU kernel has the next target's row
// in flight while the current one is written, so a draw that repeats the
// target just before it in the same pair reads that row as it was. The CPU
// twins are serial, in compacted order and in place.
//
// GPU launches, all on `stream`. An exclusive int32 scan of n items is a
// block scan (W2V_SCAN_BLOCK items per workgroup, in LDS) that leaves block
// totals, and one workgroup that scans the totals; readers add the two.
//   plan   scan of the keep flags over T + 1 items (item T is 0, so the scan
//          value there is n_kept); then one thread per position writes
//          ctok[c] and the compacted bounds [lo[c], hi[c]) of its sentence,
//          found by binary search of p in starts, zeroes loss[c >= n_kept]
//          and sets counts. Grids are sized by T; surplus waves exit.
//   step   k_w2v_window_step: one wave per centre, four per workgroup, no LDS
//          and no barrier. With D % 4 == 0 lane l holds float4 columns
//          4*(l + 64*v), v < ceil(D/256), else scalar columns l + 64*i for
//          i < 1, 2, 4 or 8 covering D. The 1 + N target words of a pair are
//          made lane-parallel (lane 0 ctx, lane d+1 draw d) and broadcast
//          target by target; the dot is a six-step xor-shuffle reduction.
//   pairs  w2v_window_pairs: the same plan, then a scan of the per-centre pair
//          counts and one thread per centre writing ctr[P], ctx[P], neg[P*N]
//          as int64 WORD ids ordered by (c, a). The buffers hold T*2W pairs.
//          This feeds the pair steps where the window step does not apply.
// `work` is w2v_window_work_words(T) int32 words on the device, contents
// irrelevant. 1 <= D <= W2V_WINDOW_MAX_DIM, T < 2^31 (for pairs T*2W < 2^31);
// callers check, and check tok and starts on the host. T == 0 is a no-op that
// still sets counts.
constexpr int W2V_WINDOW_MAX_DIM = 512;
constexpr int W2V_WINDOW_MAX_NEG = 63;
constexpr int W2V_SCAN_BLOCK = 1024;
struct W2VWindowArgs {
  const int32_t* tok;
  const int32_t* starts;
  const float* keep;  // may be null
  const float* prob;
  const int32_t* alias;
  int64_t T, S, n;
  int W, N;
  uint64_t seed;
};
inline int64_t w2v_window_work_words(int64_t T) {
  const int64_t nb = (T + W2V_SCAN_BLOCK) / W2V_SCAN_BLOCK;  // blocks over T + 1 items
  return 2 * (T + 1 + nb) + 3 * T;
}
void w2v_window_step_gpu(float* slab, int32_t plen, const W2VWindowArgs& a, int D, float lr,
                         float eps, int32_t* work, float* loss, int32_t* counts, void* stream);
void w2v_window_pairs_gpu(const W2VWindowArgs& a, int32_t* work, int64_t* ctr, int64_t* ctx,
                          int64_t* neg, int32_t* counts, void* stream);
void w2v_window_step_cpu(float* slab, int32_t plen, const W2VWindowArgs& a, int D, float lr,
                         float eps, float* loss, int32_t* counts);
void w2v_window_pairs_cpu(const W2VWindowArgs& a, int64_t* ctr, int64_t* ctx, int64_t* neg,
                          int32_t* counts);

// Matrix-factorization NZSL step: per nonzero (i, j, x):
//  w: [B][2R] row-factor rows, h: [B][2R] col-factor rows (R = rank)
//  outputs dw, dh (push deltas), loss [B] squared error
void mf_update_step_gpu(const float* w, const float* h, const float* x, float* dw, float* dh,
                        float* loss, int B, int R, float lr, float lambda, float eps,
                        void* stream);
void mf_update_step_cpu(const float* w, const float* h, const float* x, float* dw, float* dh,
                        float* loss, int B, int R, float lr, float lambda, float eps);

// MF NZSL+L2 loss reduction over B nonzeros (reference apps/mf/loss.h:
// 49-120: sum (x - w.h)^2 + lambda*(|w|^2 + |h|^2) per nonzero):
// out[0] += squared-error sum, out[1] += regularizer sum. The device sums
// are accumulated in double (acc2), which the caller rounds to fp32 once.
void mf_loss_gpu(const float* w, const float* h, const float* x, double* acc2, int B, int R,
                 float lambda, void* stream);
void mf_loss_cpu(const float* w, const float* h, const float* x, float* out2, int B, int R,
                 float lambda);

// Alias-table sampling draw (negative sampling; reference unigram table,
// word2vec.cc:125-146 — rebuilt as an O(1)-per-draw alias table):
//  prob[n] f32, alias[n] i32 built host-side; out[N] int64 drawn keys.
//  Counter-based RNG (PCG hash of (seed, index)): reproducible, stateless.
void alias_draw_gpu(const float* prob, const int32_t* alias, int64_t n, uint64_t seed,
                    int64_t N, int64_t* out, void* stream);
void alias_draw_cpu(const float* prob, const int32_t* alias, int64_t n, uint64_t seed,
                    int64_t N, int64_t* out);

// Uniform key draw that continues numpy's PCG64 bounded-integer stream bit
// for bit (ustream.h has the model). `state` is USTREAM_STATE_WORDS uint64
// words, `tmp` scratch of ustream_tmp_words(words) int64, both on the op
// device; `words` >= n is how many stream words are generated in parallel
// before compaction. Writes out[0..n) and leaves `state` where numpy would
// have left it. If fewer than n of the `words` are accepted, the last step
// continues the stream sequentially, so the result never depends on the
// slack. The device draw is two launches on `stream` and never
// synchronises; the CPU twin runs the same chunked jump-ahead and
// compaction in loops.
void uniform_draw_gpu(uint64_t* state, int64_t lo, uint32_t excl, uint32_t thr, int64_t n,
                      int64_t words, int64_t* out, int64_t* tmp, void* stream);
void uniform_draw_cpu(uint64_t* state, int64_t lo, uint32_t excl, uint32_t thr, int64_t n,
                      int64_t words, int64_t* out, int64_t* tmp);

// dst[0..n) (device) = src_host[0..n) (pinned, device-visible host memory),
// as a kernel on `stream`: for a few hundred KB of keys per step this keeps
// the upload in the compute queue, where a copy-engine transfer between two
// kernels costs a queue hand-over on either side. Returns false, with
// nothing enqueued, if src_host is not device-visible.
bool copy_keys_gpu(int64_t* dst, const int64_t* src_host, int64_t n, void* stream);

}  // namespace adapm

namespace adapm {

// ---- MFMA (matrix-core) kernels, mfma_hip.hip (gfx950
// v_mfma_f32_16x16x4_f32: exact f32 at the vector rate, ~2.4-2.8x a
// VALU f32 GEMM). GPU-only: the CPU tier uses the scalar references.

// Full-entity ComplEx eval scoring as a GEMM: scores[B][E] = Q @ Cand^T
// where Q (built by an elementwise prologue into qbuf[B*D]) is the
// (s o r) query and Cand rows are [emb(D)|accum(D)].
void kge_complex_score_mfma_gpu(const float* s, const float* r, const float* cand,
                                float* scores, float* qbuf, int B, int E, int D, void* stream);

// Rank counting for evaluation (k_mfma_rank_count): score a tile, count the
// winners, write no score matrix.
//   counts[b] += #{ e in [0, E) : dot_K(Q[b], C[e]) > base[b]  or  isnan(dot_K(Q[b], C[e])) }
//   Q: [B] rows, row stride qstride >= K floats, first K used
//   C: [E] rows, row stride cstride >= K floats, first K used
//   base: [B] float    counts: [B] int32, accumulated (the caller zeroes it; chunks add up)
// The comparison is strict: a score equal to base does not count. Any
// K >= 1; row offsets are 64-bit. max_blocks caps the grid (0: the launcher's
// own cap); a workgroup adds to a row of counts at most once. B < 1 or E < 1
// is a no-op. The CPU twin sums each dot as a std::fmaf chain in ascending k.
void rank_count_gpu(const float* Q, const float* C, const float* base, int32_t* counts, int B,
                    int E, int K, int qstride, int cstride, int max_blocks, void* stream);
void rank_count_cpu(const float* Q, const float* C, const float* base, int32_t* counts, int B,
                    int E, int K, int qstride, int cstride);

// Pair scores: out[p] = dot_K(Q[owner[p]], C[p]) for p in [0, P), owner int32
// in [0, B). out[p] carries the bits of the score rank_count computes for
// that (query, candidate) pair wherever the candidate sits in its tiles, so
// a base taken from here never counts its own candidate, and a competitor is
// above base here exactly when rank_count counted it.
void pair_scores_gpu(const float* Q, const float* C, const int32_t* owner, float* out, int P,
                     int K, int qstride, int cstride, void* stream);
void pair_scores_cpu(const float* Q, const float* C, const int32_t* owner, float* out, int P,
                     int K, int qstride, int cstride);

// Batched varying-M grouped GEMM (triples sorted by relation; group g =
// rows [starts[g], starts[g+1]), relation matrix g at Rm + g*rstride):
//   mode 0: Out[row] = S_g @ R_g        (U = R^T e_s per row)
//   mode 1: Out[row] = W_g @ R_g^T      (de_s raw)
//   mode 2: Out[g]   = S_g^T @ W_g      (dR raw, [G][D*D])
void mfma_grouped_gemm_gpu(const float* S, const float* W, const float* R, float* out,
                           const int* starts, int G, int D, int sstride, int wstride,
                           int64_t rstride, int out_rstride, int64_t ostride, int mode,
                           int total_tiles, void* stream);

// per-triple middle phase of the grouped RESCAL step (scores, object
// grads with fused AdaGrad, W accumulation) given precomputed U
void rescal_mid_gpu(const float* U, const float* o, const float* neg, float* do_, float* dneg,
                    float* Wm, float* loss, int B, int N, int D, float lr, float eps,
                    void* stream);

// AdaGrad epilogue: out rows = [ -lr*g/sqrt(G+g^2+eps) | g^2 ] from a
// raw-gradient buffer and the accumulator half of the pulled rows
void adagrad_rows_gpu(const float* grad, const float* rows, float* out, int64_t n_rows,
                      int dvals, int gstride, int rstride, float lr, float eps, void* stream);

// middle phase of the grouped RESCAL sides step, given U = S R (u_b) and
// V = O R^T (v_b), both [B][D]. Object pass: scores u_b . o_j, dneg_o with
// fused AdaGrad, Wm[b] = c_0 o + sum_j c_j o'_j, dO0[b] = c_0 u_b (the raw
// gradient of the positive object so far). Subject pass: scores s'_j . v_b,
// dneg_s with fused AdaGrad, Zm[b] = sum_j a_j s'_j. Wm, Zm, dO0 are [B][D].
void rescal_mid_sides_gpu(const float* U, const float* V, const float* o, const float* neg_o,
                          const float* neg_s, float* dneg_o, float* dneg_s, float* Wm,
                          float* Zm, float* dO0, float* loss, int B, int N, int NS, int D,
                          float lr, float eps, void* stream);

// AdaGrad epilogue of a summed gradient: as adagrad_rows_gpu with
//   g = ga[r][k] + gb[r][k] + gamma * count_r * rows[r][k]
// gb may be null (no second buffer). count_r is starts[r+1] - starts[r] with
// `starts` (device, n_rows + 1 ints), else 1; a row of count 0 gets [0 | 0].
// `out` must not overlap ga or gb.
void adagrad_rows_sum_gpu(const float* ga, const float* gb, const float* rows, float* out,
                          const int* starts, int64_t n_rows, int dvals, int gastride,
                          int gbstride, int rstride, float lr, float eps, float gamma,
                          void* stream);

}  // namespace adapm
