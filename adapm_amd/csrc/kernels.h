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
#include <cstdint>

namespace adapm {

// The ComplEx and SGNS step kernels (classic and fused) hold a row's lanes
// in registers, at most 8 per thread of a 256-thread workgroup. ComplEx has
// D/2 lanes per row, SGNS D. Callers refuse longer rows before launching;
// the CPU twins have no such limit.
constexpr int STEP_MAX_LANES = 8 * 256;

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
// kernel itself, which is what makes the results the same bit for bit. No
// dropout (off by default in the reference).
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
