/*
 * smatrix_batch.h -- additive batched entry points (no reference counterpart as
 * functions; each applies the reference's per-call semantics, src/smatrix.c:174-256,
 * to n (x,y[,value]) triples at once -- the form the HIP kernels consume).
 *
 * Contract (SURVEY.md 8a "batch semantics"):
 *  - the final table state equals applying the n ops one by one in SOME order the
 *    reference's threads could have produced; row sizes and `used` counters are
 *    exactly the reference's (they do not depend on the order);
 *  - incr/decr: out[i] is the value after op i in that order (exact for unique
 *    keys; for duplicates the largest out equals the final value);
 *  - set: duplicates of one (x,y) inside a batch resolve to the HIGHEST index;
 *    out[i] = v[i];
 *  - a batch of one op, or any stream applied one op per call, reproduces the
 *    reference's table bytes slot for slot.
 *
 * Two flavours: host pointers (staged through HBM by the library; calls above two chunks of 2^21 ops -- SMATRIX_HOST_CHUNK_LG --
 * run as a three-stage pipeline: the caller's arrays are copied into pinned memory by a pool of threads and uploaded while the
 * kernels of the previous chunk run and the results of the one before travel back; a write batch's chunks are applied in order,
 * so the call behaves like ONE batch -- set: the later op still wins; a chunk whose amounts v[] are all one value is filled on
 * the device instead of uploaded.  2^24-op calls: 3.1-3.5 G incr/s, 4.4-5.0 G get/s, PCIe
 * included; this is the shape a JNI / Ruby batch binding has, cf. src/smatrix_jni.c:95-111) and `_dev`
 * (pointers are device memory on the matrix's GPU; work is enqueued on
 * `hip_stream` -- a hipStream_t passed as void*; NULL = the legacy default stream, i.e. what
 * `torch.cuda.current_stream().cuda_stream` is unless the caller switched streams, so inputs
 * produced by earlier work on that stream are ordered before the kernels that read them.
 * Results are complete in stream order: writers return after their last round has
 * finished on that stream, get/rowlen/getrow may return as soon as they are enqueued;
 * with hip_stream == NULL every call synchronises before returning).
 * ORDERING: the library's lock serialises host code only.  All calls on one handle must reach the GPU in one order:
 * use ONE stream per handle, or order the streams yourself (events) -- a get/rowlen/getrow enqueued on stream A
 * and a later write on stream B would otherwise race on the tables (a write may grow rows, recycle their old
 * blocks and replace the directory).  hip_stream == NULL and the host-pointer calls always synchronise.
 * Return value: 0 on success; failures abort like the scalar API.
 * n must be < 2^32.
 */
#ifndef SMATRIX_BATCH_H
#define SMATRIX_BATCH_H

#include "smatrix.h"

#ifdef __cplusplus
extern "C" {
#endif

/* op codes for smatrix_apply_batch* */
enum { SMATRIX_OP_GET = 0, SMATRIX_OP_SET = 1, SMATRIX_OP_INCR = 2, SMATRIX_OP_DECR = 3 };

int smatrix_apply_batch(smatrix_t* self, int op, size_t n, const uint32_t* x,
                        const uint32_t* y, const uint32_t* v, uint32_t* out);
int smatrix_get_batch(smatrix_t* self, size_t n, const uint32_t* x, const uint32_t* y, uint32_t* out);
int smatrix_set_batch(smatrix_t* self, size_t n, const uint32_t* x, const uint32_t* y,
                      const uint32_t* v, uint32_t* out);
int smatrix_incr_batch(smatrix_t* self, size_t n, const uint32_t* x, const uint32_t* y,
                       const uint32_t* v, uint32_t* out);
int smatrix_decr_batch(smatrix_t* self, size_t n, const uint32_t* x, const uint32_t* y,
                       const uint32_t* v, uint32_t* out);
int smatrix_rowlen_batch(smatrix_t* self, size_t n, const uint32_t* x, uint32_t* out);
/* row r writes at most offsets[r+1]-offsets[r] pairs at ret + 2*offsets[r] (uint32 units),
 * in table slot order; counts[r] = pairs written.  offsets has n+1 entries. */
int smatrix_getrow_batch(smatrix_t* self, size_t n, const uint32_t* x, const uint64_t* offsets,
                         uint32_t* ret, uint32_t* counts);

/* device-pointer flavours (d_v is not read by get).  out / d_out may be NULL in every write call when the results are not
 * wanted: the table ends in exactly the same state, the result stores are skipped, and updates of a column-0 cell (the CF
 * example's per-item totals, examples/cf_recommender.c:38) are made with one 64-bit add instead of a compare-and-swap
 * loop -- under heavy contention on a hot item's total that is the difference between 24 ms and 3 ms per 2^25 ops. */
int smatrix_apply_batch_dev(smatrix_t* self, int op, size_t n, const uint32_t* d_x,
                            const uint32_t* d_y, const uint32_t* d_v, uint32_t* d_out,
                            void* hip_stream);

/* The same on ONE device array of n records {x, y} (width 2, get only) or {x, y, v} (width 3): the form
 * in which the sharded exchange delivers a batch (include/smatrix_shard.h) -- no unpacking pass. */
int smatrix_apply_packed_dev(smatrix_t* self, int op, size_t n, const uint32_t* d_records, uint32_t width,
                             uint32_t* d_out, void* hip_stream);
int smatrix_rowlen_batch_dev(smatrix_t* self, size_t n, const uint32_t* d_x, uint32_t* d_out,
                             void* hip_stream);
int smatrix_getrow_batch_dev(smatrix_t* self, size_t n, const uint32_t* d_x,
                             const uint64_t* d_offsets, uint32_t* d_ret, uint32_t* d_counts,
                             void* hip_stream);

/* CF-recommender read path, fused (the reference's documented production use,
 * examples/cf_recommender.c:50-86): for each item a, every neighbour (b, cc) of getrow(a) gets
 *   score = cc / (sqrt(get(a,0)) * sqrt(get(b,0)))      in double,
 * with the example's guards (get(b,0) == 0 -> 1; den == 0 -> 0; cc > den -> 0).  Neighbours come in
 * table slot order; item i writes at most offsets[i+1]-offsets[i] of them at ids/scores + offsets[i];
 * counts[i] = neighbours written.  Column 0 holds the per-item totals, so quirks Q1/Q2 apply. */
int smatrix_cf_neighbors_batch(smatrix_t* self, size_t n, const uint32_t* items, const uint64_t* offsets,
                               uint32_t* ids, double* scores, uint32_t* counts);
int smatrix_cf_neighbors_batch_dev(smatrix_t* self, size_t n, const uint32_t* d_items,
                                   const uint64_t* d_offsets, uint32_t* d_ids, double* d_scores,
                                   uint32_t* d_counts, void* hip_stream);

/* The same read path, but only the k <= 64 BEST neighbours of each item leave the GPU (what a recommender serves):
 * best score first, equal scores in table slot order; the candidates and the score are exactly those above (the
 * (0,total) entry of the row included, as in the example's loop).  ids / scores hold n*k entries, item i's at
 * [i*k, i*k + counts[i]); counts[i] = min(k, entries of the row).  Returns -1 for k == 0 or k > 64. */
int smatrix_cf_topk_batch(smatrix_t* self, size_t n, const uint32_t* items, uint32_t k, uint32_t* ids, double* scores,
                          uint32_t* counts);
int smatrix_cf_topk_batch_dev(smatrix_t* self, size_t n, const uint32_t* d_items, uint32_t k, uint32_t* d_ids,
                              double* d_scores, uint32_t* d_counts, void* hip_stream);

/* Session recommendations ("people who viewed these also viewed"): the k <= 64 best items for each session (a user's or
 * a basket's items), the whole query fused on the GPU.  Session s is items[offsets[s] .. offsets[s+1]) (n_sessions + 1
 * offsets; a session holds fewer than 2^32 items).
 *   items      duplicates count once, at their first position; an item with no row contributes nothing.
 *   candidates every b that is the key of a non-empty cell in the row of some session item a, with b != 0 (column 0
 *              holds the totals) and b not itself an item of the session (a row can hold its own id: the import counts
 *              an id that occurs twice in a session against itself).
 *   score(b)   the sum over the session's distinct items a whose row holds b of cf_cosine(a, b), each term exactly as
 *              smatrix_cf_neighbors_batch computes it (get(b,0) == 0 -> 1; den == 0 -> 0; cc > den -> 0), added in
 *              session order (first positions) from 0.0, in double: bit-equal to a left-to-right sum of those doubles.
 *   output     the k best candidates, score descending, equal scores by ascending id: the result depends only on the
 *              matrix's contents.  ids / scores hold n_sessions*k entries, session s's at [s*k, s*k + counts[s]);
 *              counts[s] = min(k, candidates).  The host flavour zero-fills the unused entries; _dev leaves them.
 * Returns -1 for k == 0, k > 64 or n_sessions >= 2^32, 0 otherwise.  Takes the matrix lock and sees values the scalar
 * calls still hold in the host mirror; file-backed matrices work unchanged.  The same contents and input give the same
 * bytes on every call.
 * _dev: all arrays in device memory, on hip_stream (NULL: the legacy default stream, synchronised before returning).  The
 * matrix's scratch is shared by all calls: a call's work waits on the stream for the previous call's, whatever its stream. */
int smatrix_cf_recommend_batch(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                               uint32_t k, uint32_t* ids, double* scores, uint32_t* counts);
int smatrix_cf_recommend_batch_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                   uint32_t k, uint32_t* d_ids, double* d_scores, uint32_t* d_counts, void* hip_stream);

/* Session recommendations with "not these" and recency: smatrix_cf_recommend_batch with per-position weights, a per-session
 * exclusion list (a user's own history) and a deny bitmap for all sessions (out of stock, delisted), all applied on the GPU
 * BEFORE the k best are taken, so k valid results come back however many candidates are filtered.  What is not said here is
 * smatrix_cf_recommend_batch's contract; with weights, ex_offsets, ex_items, deny_bits NULL and deny_n 0 the call writes its bytes.
 *   weights    NULL (every weight 1.0), or one double per entry of items: weights[offsets[s] + i] belongs to
 *              items[offsets[s] + i].  A distinct item has the weight at its FIRST position; later occurrences are ignored,
 *              weight included.  score(b) = the left-to-right sum from 0.0, in session order, of w_a * cf_cosine(a, b), the
 *              product rounded to double on its own before it is added; w == 1.0 gives the unweighted bytes.  Every weight
 *              must be finite and >= 0 (-0.0 acts as 0.0).  An item of weight 0 is still an item of the session: it is not
 *              recommended, and the keys of its row are candidates with a term of 0.0.
 *   ex_*       both NULL, or ex_offsets has n_sessions + 1 entries and session s is never given
 *              ex_items[ex_offsets[s] .. ex_offsets[s+1]) (fewer than 2^32 ids a list).  An id may be repeated, 0 or absent
 *              from the matrix (no effect), or an item of the session, which stays an item: its row is scanned and its
 *              weight counts.  The rows of excluded ids are not read.
 *   deny_*     deny_bits NULL with deny_n == 0, or a bitmap over the ids 0 .. deny_n - 1 (deny_n <= 2^32, (deny_n + 31) / 32
 *              words): id b < deny_n is denied when bit b & 31 of word b >> 5 is set, ids >= deny_n are allowed.  A denied id
 *              is given to no session; as an item of a session it contributes like any other.
 *   counts     excluded and denied ids do not count: counts[s] = min(k, candidates left).
 * Returns -1 for k == 0, k > 64, n_sessions >= 2^32, deny_n > 2^32, deny_bits NULL with deny_n != 0, exactly one of ex_offsets /
 * ex_items NULL, or a weight that is negative, NaN or infinite: the host flavour checks the weights before it touches the device
 * and leaves the outputs as they were, _dev finds them on the device and leaves the outputs' contents unspecified.  0 otherwise.
 * Memory beyond smatrix_cf_recommend_batch's: one more slot per exclusion-list entry in the session's table (a session's table
 * has room for its candidates, its items and its list, so a small session with a long list is summed in device memory, 20
 * bytes a slot, not in LDS); the host flavour also holds device copies of the three inputs for the call. */
int smatrix_cf_recommend_filtered(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                                  const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                                  const uint32_t* deny_bits, uint64_t deny_n, uint32_t k, uint32_t* ids, double* scores,
                                  uint32_t* counts);
int smatrix_cf_recommend_filtered_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                      const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                      const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t k, uint32_t* d_ids,
                                      double* d_scores, uint32_t* d_counts, void* hip_stream);

/* Session recommendations by another similarity than the cosine, and with shrinkage: smatrix_cf_recommend_filtered with the
 * score of a pair chosen by the caller.  What is not said here is smatrix_cf_recommend_filtered's contract, word for word:
 * candidates, first positions, weights (w_a * score, the product rounded on its own), exclusion lists, the deny bitmap, counts,
 * the result order (score descending, equal scores by ascending id), tiers, locks, streams, memory.
 *   score      of the pair (b, cc) in the row of session item a, in place of cf_cosine(a, b).  ta = what smatrix_get(a, 0)
 *              returns (0 without a row or a head pair), tb = smatrix_get(b, 0) with 0 counted as 1; A, B, c = ta, tb, cc as
 *              doubles (exact).  Everything is IEEE double, sqrt * + - / correctly rounded:
 *                  if (ta == 0) score = 0.0;                          every measure
 *                  base = SMATRIX_SIM_COSINE   sqrt(A) * sqrt(B)
 *                         SMATRIX_SIM_JACCARD  (A + B) - c            Jaccard / Tanimoto on co-occurrence counts
 *                         SMATRIX_SIM_LIFT     A * B                  lift but for the constant factor: punishes popular b harder
 *                  den   = base + shrink;                             base rounded to double ON ITS OWN, then one add: never a
 *                                                                     fused multiply-add
 *                  score = (den != 0.0 && !(c > den)) ? c / den : 0.0;
 *              Scores lie in [0, 1] (a negative Jaccard denominator fails c > den and gives 0).  A session item with ta == 0 is
 *              still an item: the keys of its row are candidates with a term of 0.0.
 *   shrink     one finite double >= 0 for the call (-0.0 acts as 0.0), added to every denominator: a pair seen once between two
 *              items seen once (cc = ta = tb = 1: cosine 1.0, the best possible score) no longer outranks a pair seen 200 times
 *              between two common items.
 * sim == SMATRIX_SIM_COSINE with shrink == 0 writes smatrix_cf_recommend_filtered's bytes (the same code path).
 * Returns -1 for smatrix_cf_recommend_filtered's refusals, an unknown sim, and a shrink that is negative, NaN or infinite: shrink
 * is a host scalar, so BOTH flavours refuse it before the device is touched and leave the outputs as they were.  0 otherwise.
 * smatrix_cf_neighbors_batch and smatrix_cf_topk_batch stay cosine-only: an item's best neighbours by another measure are the
 * result of this call for the session of that one item. */
enum { SMATRIX_SIM_COSINE = 0, SMATRIX_SIM_JACCARD = 1, SMATRIX_SIM_LIFT = 2 };
int smatrix_cf_recommend_sim(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                             const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                             const uint32_t* deny_bits, uint64_t deny_n, int sim, double shrink, uint32_t k, uint32_t* ids,
                             double* scores, uint32_t* counts);
int smatrix_cf_recommend_sim_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                 const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                 const uint32_t* d_deny_bits, uint64_t deny_n, int sim, double shrink, uint32_t k,
                                 uint32_t* d_ids, double* d_scores, uint32_t* d_counts, void* hip_stream);

/* Diverse results: smatrix_cf_recommend_sim with at most `cap` results of a session from one group -- brand, category, seller; the
 * library does not care which.  The rule runs on the GPU over the session's WHOLE ranking, before the cut at k: a session whose best
 * 64 candidates come from three brands still gets its 10 results.  Everything not said here is smatrix_cf_recommend_sim's contract,
 * word for word: sessions, first positions, candidates, the score of a pair, weights, exclusion lists, the deny bitmap, tiers, locks,
 * the mirror, streams, scratch, k <= 64.
 *   group_of   one uint32 per id 0 .. group_n - 1, group_n <= 2^32: candidate b belongs to group group_of[b].  An id >= group_n, or
 *              one whose entry is SMATRIX_GROUP_NONE, is UNGROUPED: it is never capped and consumes nobody's quota.  Every other
 *              32-bit value is a group id, 0 and 0xFFFFFFFE included.
 *   cap        1 <= cap <= 64: the most results of one session that may share a group.  One number for the call.
 *   result     walk the session's candidates that are left in the sim call's result order (score descending, equal scores by
 *              ascending id); take a candidate iff it is ungrouped or fewer than cap candidates already taken share its group; stop
 *              at k.  ids / scores hold the taken ones in walk order, each score the sim call's bytes for that id; counts[s] is
 *              their number, which may be < k although the session has >= k candidates.  In closed form: a grouped candidate
 *              survives iff fewer than cap candidates of its own group precede it in the result order, and the result is the first k
 *              survivors.  A session item, an excluded id and a denied id are no candidates: they consume no quota.
 *   unused     entries beyond counts[s]: the host flavour zero-fills them, _dev leaves them.
 *   no grouping group_of NULL with group_n == 0 writes smatrix_cf_recommend_sim's bytes through the same launches; so does a cap >= k
 *              with a map given (such a quota refuses nobody before the cut).
 * Deterministic: the same contents and input give the same bytes; nothing depends on slot order, lane order or the tier.
 * Cost beyond the sim call's: one 4-byte gather from group_of per candidate, then rounds over the session's table -- a round looks at
 * the 64 best candidates still alive, takes what the quotas allow and strikes out those 64 and every candidate of a group that is
 * full now.  A round's first candidate is always taken: at most k rounds, one or two for a typical session.  A session of the
 * global tier is ended by one workgroup over its whole table (as smatrix_cf_rank's).  The host flavour stages group_of once per call.
 * Returns -1 for smatrix_cf_recommend_sim's refusals, word for word, and for cap == 0, cap > 64, group_n > 2^32 and group_of NULL
 * with group_n != 0 (before the device is touched, outputs as they were, both flavours).  0 otherwise.
 * Not here: a cap per group (an array of quotas) and the sharded matrix. */
#define SMATRIX_GROUP_NONE 0xFFFFFFFFu
int smatrix_cf_recommend_grouped(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                                 const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                                 const uint32_t* deny_bits, uint64_t deny_n, const uint32_t* group_of, uint64_t group_n,
                                 uint32_t cap, int sim, double shrink, uint32_t k, uint32_t* ids, double* scores,
                                 uint32_t* counts);
int smatrix_cf_recommend_grouped_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                     const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                     const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_group_of, uint64_t group_n,
                                     uint32_t cap, int sim, double shrink, uint32_t k, uint32_t* d_ids, double* d_scores,
                                     uint32_t* d_counts, void* hip_stream);

/* A long ranked list: smatrix_cf_recommend_sim with up to SMATRIX_DEEP_MAX results per session -- the candidate stage in front of a
 * second-stage ranker, a re-ranking by price or margin on the caller's side, recall@k beyond 64 from one call.  Everything is
 * smatrix_cf_recommend_sim's contract, word for word, except the bound on k: sessions, first positions, candidates, the score of a
 * pair, weights, exclusion lists, the deny bitmap, the result order (score descending, equal scores by ascending id), tiers, locks,
 * the mirror, streams, scratch; the host flavour zero-fills the entries beyond counts[s], _dev leaves them.
 *   k          1 <= k <= SMATRIX_DEEP_MAX.  ids and scores hold n_sessions * k entries (the product is taken in 64 bits); session
 *              s's are [s*k, s*k + counts[s]), counts[s] = min(k, the candidates left).
 *   k <= 64    the call IS smatrix_cf_recommend_sim: the same launches, the same bytes in all three outputs.
 *   k > 64     entry r < 64 of a session has the bytes smatrix_cf_recommend_sim with k = 64 writes there, and for every r
 *              smatrix_cf_rank with the same arguments answers the target ids[s*k + r] with the rank r and the bytes of
 *              scores[s*k + r].
 * Deterministic: the same contents and input give the same bytes; nothing depends on slot order, lane order, the tier or the number of
 * passes a selection took.
 * Cost beyond the sim call's, with k > 64: per session a radix select of the k-th best (score, id) over its table -- a pass per byte
 * in which the candidates' keys still differ, at most 12, each a pass over the table --, then a sort of the <= 1024 entries at or
 * above it.  A session of the global tier is ended by one workgroup over its whole table (as smatrix_cf_rank's).
 * Returns -1 for smatrix_cf_recommend_sim's refusals, word for word but for the bound on k, and for k == 0 and k > SMATRIX_DEEP_MAX
 * (both flavours before the device is touched, outputs as they were; a bad weight as there).  0 otherwise.
 * Not here: fill lists and group quotas beyond 64 results (smatrix_cf_recommend_fill and smatrix_cf_recommend_grouped keep a
 * session's results in the 64 lanes of a wave), the item-neighbour calls (smatrix_cf_topk_batch stays at k <= 64), and the sharded
 * matrix. */
#define SMATRIX_DEEP_MAX 1024u
int smatrix_cf_recommend_deep(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                              const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                              const uint32_t* deny_bits, uint64_t deny_n, int sim, double shrink, uint32_t k, uint32_t* ids,
                              double* scores, uint32_t* counts);
int smatrix_cf_recommend_deep_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                  const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                  const uint32_t* d_deny_bits, uint64_t deny_n, int sim, double shrink, uint32_t k,
                                  uint32_t* d_ids, double* d_scores, uint32_t* d_counts, void* hip_stream);

/* The rank of given items in a session's ranking: where a held-out item lands among ALL the session's candidates, not only among
 * the k <= 64 best -- what hit-rate@k, MRR and the loss of a truncated copy are computed from.  Everything up to and including
 * shrink is smatrix_cf_recommend_sim's contract, word for word: sessions, first positions, candidates, the score of a pair, weights,
 * exclusion lists, the deny bitmap, tiers, locks, the mirror, streams, scratch.  There is no k.
 *   targets    session s asks about targets[t_offsets[s] .. t_offsets[s+1]) (n_sessions + 1 non-decreasing offsets).  A list may
 *              be empty and may hold an id more than once; every entry is answered on its own: ranks[j] and scores[j] answer
 *              targets[j].  The targets are looked up, never entered: they change no table, no tier and no other answer.
 *   answer     when targets[j] is a candidate that is left (the key of a cell in some session item's row, not 0, not an item of
 *              the session, not on its exclusion list, not denied): scores[j] = its sum, the bytes smatrix_cf_recommend_sim returns
 *              for it; ranks[j] = the number of candidates left that come before it in the result order (score descending, equal
 *              scores by ascending id).  So wherever smatrix_cf_recommend_sim with the same arguments returns ids[s*k + r] == t,
 *              the rank of t is r, and the numbering goes on past 64.  For anything else (the id 0, an id in no scanned row, an
 *              item of the session, an excluded or denied id): ranks[j] = SMATRIX_RANK_NONE, scores[j] = 0.0.
 *   n_candidates[s] = the candidates left, uncapped (smatrix_cf_recommend_sim's counts[s] is min(k, this)); written for every
 *              session, also for one with no targets or no rows.
 * All three outputs are required, and every entry the call owns is defined when it returns 0.  The host flavour reads and writes
 * only the entries t_offsets[0] <= j < t_offsets[n_sessions] of targets, ranks and scores (as items from offsets[0]).
 * Cost: the recommend call's up to the selection, then one pass over the session's table per 64 targets; no sort, no merge.
 * Returns -1 for smatrix_cf_recommend_sim's refusals but those of k (an unknown sim and a bad shrink in both flavours before the
 * device is touched, outputs as they were; a bad weight as there: the host flavour before the device is touched, _dev on the device
 * with the outputs' contents unspecified) and for t_offsets or targets NULL.  0 otherwise, n_sessions == 0 included. */
#define SMATRIX_RANK_NONE 0xFFFFFFFFu
int smatrix_cf_rank(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                    const uint64_t* ex_offsets, const uint32_t* ex_items, const uint32_t* deny_bits, uint64_t deny_n, int sim,
                    double shrink, const uint64_t* t_offsets, const uint32_t* targets, uint32_t* ranks, double* scores,
                    uint32_t* n_candidates);
int smatrix_cf_rank_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                        const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                        const uint32_t* d_deny_bits, uint64_t deny_n, int sim, double shrink, const uint64_t* d_t_offsets,
                        const uint32_t* d_targets, uint32_t* d_ranks, double* d_scores, uint32_t* d_n_candidates,
                        void* hip_stream);

/* Why an item was recommended: each session item's share of a candidate's score ("because you viewed X and Y").  A score of
 * smatrix_cf_recommend_sim is a left-to-right sum of w_a * score(a, b) over the session's distinct items; this call returns the
 * terms of that sum for the targets the caller names, one per (target, session position), made by the library's own rules.
 * Sessions, weights, sim and shrink are smatrix_cf_recommend_sim's, word for word; targets and t_offsets are smatrix_cf_rank's (a
 * list may be empty and may hold an id more than once; every entry is answered on its own).  L_s = the length of session s, T_s =
 * the number of its targets.
 *   layout     dense, one entry per (target, position): E_s = the sum of T_s' * L_s' over the sessions before s; target number j
 *              of session s (counted from 0 within the session) and position i < L_s own entry E_s + j * L_s + i of terms and of
 *              cc, so session s's block reshapes to (T_s, L_s).  The host flavour computes E_s itself and writes
 *              terms[0 .. E_n) and cc[0 .. E_n); it reads items, weights and targets from offsets[0] and t_offsets[0] on, as
 *              smatrix_cf_rank does.  _dev: the caller passes d_e_offsets (n_sessions + 1 entries, d_e_offsets[s] = E_s) and
 *              total = E_n (as d_op_offsets / total_ops of smatrix_cf_import_sessions_dev).  The kernels write nothing outside
 *              [0, total) of the two outputs whatever d_e_offsets holds; with offsets that are not the E_s above the contents are
 *              unspecified.
 *   answer     for target t and position i holding item a.  terms = +0.0 and cc = 0 when t == 0, when a occurs earlier in the
 *              session (first positions count, exactly, at every session length), when a has no row, or when a's row has no
 *              cell with key t.  Otherwise cc = what smatrix_get(a, t) returns, and terms = w * score: score is
 *              smatrix_cf_recommend_sim's score of the pair (t, cc) in row a for (sim, shrink) -- ta == 0 scores 0, tb == 0
 *              counts as 1, base rounded on its own before shrink is added --, w the weight at that position (1.0 with weights
 *              NULL), the product rounded to double on its own.  A weight of -0.0 acts as 0.0: no entry is ever -0.0.  A dead
 *              cell (cc == 0) gives +0.0.
 *   no filters there is no exclusion list and no deny bitmap: an explanation does not depend on whether t would be served, and a
 *              target that is itself an item of the session is answered like any other.
 * What ties it to the rest: wherever smatrix_cf_rank with the same sessions, weights, sim and shrink (and any filters) answers
 * target t of session s with a rank, the left-to-right sum from 0.0 of that target's L_s terms has exactly the bytes of its
 * scores[j] -- the bytes of smatrix_cf_recommend_sim's score for t.  One exception: a row that holds a key twice (SURVEY.md quirk
 * Q4, a reloaded file); the recommend call adds both cells' terms, this call reports the cell smatrix_get finds.
 * Cost: sum of T_s * L_s look-ups, one per entry, after a pre-pass of one look-up per session entry and one per target.  The
 * pre-pass finds the first positions by the quadratic wave compare of smatrix_cf_recommend_batch's tier pass (every position
 * against all earlier ones, 64 at a time: L_s * (L_s + 1) / 2 compares), here without its cut at 8192 ids.  Scratch: 8 bytes per
 * session entry and 8 bytes per target; the host flavour also holds device copies of its inputs and outputs for the call.  No
 * session table is built.  _dev reads d_offsets[n_sessions] and d_t_offsets[n_sessions] back (16 bytes) to size the scratch.
 * Locks, the mirror and streams are smatrix_cf_rank's: the matrix lock for the call, scalar writes still in the host mirror
 * written back first, the scratch ordered behind the previous read-path call whatever its stream, hip_stream == NULL
 * synchronises; file-backed matrices work unchanged.  The matrix is not modified.  Deterministic: the same contents and input give
 * the same bytes.
 * Returns -1 for n_sessions >= 2^32, an unknown sim, a shrink that is negative, NaN or infinite (both flavours, before the device
 * is touched, outputs as they were), t_offsets, targets, terms or cc NULL, _dev: d_e_offsets NULL, and a weight that is negative,
 * NaN or infinite: the host flavour checks the weights before it touches the device and leaves the outputs as they were, _dev
 * finds them on the device (one 4-byte read-back) and leaves the outputs' contents unspecified.  0 otherwise, n_sessions == 0 and
 * total == 0 included. */
int smatrix_cf_explain(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items, const double* weights,
                       int sim, double shrink, const uint64_t* t_offsets, const uint32_t* targets,
                       double* terms, uint32_t* cc);
int smatrix_cf_explain_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                           const double* d_weights, int sim, double shrink, const uint64_t* d_t_offsets,
                           const uint32_t* d_targets, const uint64_t* d_e_offsets, uint64_t total,
                           double* d_terms, uint32_t* d_cc, void* hip_stream);

/* The most popular items: the n ids with the largest totals (column 0), selected on the GPU over the whole directory -- what a
 * short result is back-filled with (smatrix_cf_recommend_fill below), without an export of the matrix to the host.
 *   candidates every id x != 0 for which smatrix_row_info(x) returns 1, with total(x) >= max(min_total, 1) and x not denied.
 *              total(x) = what smatrix_get(x, 0) returns once the mirror is written back: a row without a head pair has total 0
 *              and is no candidate, neither is an empty row (quirk Q3, set(x, 0, 0) on a new row) nor one whose head was
 *              decremented to 0.  The deny bitmap is smatrix_cf_recommend_filtered's, bit for bit: ids >= deny_n are allowed,
 *              deny_bits NULL goes with deny_n == 0.
 *   order      by the key RkValue::make(x, total) of kernels/rank_key.hpp: total descending, equal totals by ascending id.  Keys
 *              are unique, so the result depends on the matrix's contents alone, not on directory order, insertion history or growth.
 *   output     the min(n, candidates) best, best first: ids[i] / totals[i], *n_found their number (a DEVICE pointer in _dev).  The
 *              host flavour zero-fills the unused entries of ids and totals; _dev leaves them.
 * Returns -1, outputs as they were and the device untouched, for n == 0, n > SMATRIX_POPULAR_MAX, deny_n > 2^32, deny_bits NULL
 * with deny_n != 0, and ids, totals or n_found NULL.  0 otherwise, an empty matrix included (n_found = 0).
 * How: a key per directory slot (one directory pass, one head-cell gather per row), a device-wide MSB radix select over the keys
 * -- per pass a streaming 256-bin histogram and a one-wave pick, from the highest byte that is not 0 in every key down, so totals
 * below 256 start at byte 4 of 8 --, the keys at or above the threshold collected with one atomic add per workgroup, and one
 * workgroup that sorts them in LDS.  Everything between the first kernel and the stores is decided on the device: _dev makes no
 * read-back at all.  Scratch: 8 bytes per directory slot, 8 n bytes and a control block of 8 KiB.
 * Locks, the mirror, streams and scratch are the read path's (smatrix_cf_rank's): the matrix lock for the call, scalar writes still
 * in the host mirror written back first, the scratch ordered behind the previous read-path call whatever its stream, hip_stream ==
 * NULL synchronises; file-backed matrices work unchanged.  The matrix is not modified.  Deterministic. */
#define SMATRIX_POPULAR_MAX 4096u
int smatrix_cf_popular(smatrix_t* self, const uint32_t* deny_bits, uint64_t deny_n, uint32_t min_total,
                       uint32_t n, uint32_t* ids, uint32_t* totals, uint32_t* n_found);
int smatrix_cf_popular_dev(smatrix_t* self, const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t min_total,
                           uint32_t n, uint32_t* d_ids, uint32_t* d_totals, uint32_t* d_n_found, void* hip_stream);

/* The trending items: the n ids whose totals (column 0) in `now` grew most against a scaled baseline taken from a second matrix,
 * `base` -- the matrix of an older window, as smatrix_cf_import_events / smatrix_merge_scaled leave one --, joined and selected on
 * the GPU with no export of either matrix.  The ids are a fill list for smatrix_cf_recommend_fill as they stand.
 *   candidates every id x != 0 for which smatrix_row_info(now, x) returns 1, x not denied, with
 *                T = smatrix_get(now, x, 0) >= max(min_total, 1);
 *                B = smatrix_get(base, x, 0): 0 for an id without a row in base, a row without a head pair, or a head decremented to 0;
 *                E = floor(B * num / den), computed in 64 bits: smatrix_merge_scaled's transform, with its 1 <= num <= den;
 *                T > E, and the gain G = T - E >= max(min_gain, 1).
 *              The deny bitmap is smatrix_cf_recommend_filtered's, bit for bit.  An id that only base holds is no candidate.
 *   score      an IEEE double; G and E are converted exactly and each operation is rounded on its own (no fused multiply-add):
 *                D = (double)E + shrink; if (D == 0.0) D = 1.0;      (a new item with shrink == 0: the read path's tb == 0 -> 1)
 *                SMATRIX_TREND_GAIN    (double)G          absolute gain: mostly hands back the popular items
 *                SMATRIX_TREND_RATIO   G / D              relative growth, smoothed by shrink
 *                SMATRIX_TREND_ZSCORE  G / sqrt(D)        a Poisson z-score with smoothing
 *              Every candidate's score is finite and greater than 0.
 *   order      score descending, equal scores by ascending id: the key RkCosine::make(x, score bits) of kernels/rank_key.hpp.  Keys
 *              are unique, so the result depends on the two matrices' contents alone, not on directory order, insertion history
 *              or growth.
 *   output     the min(n, candidates) best, best first: ids[i], scores[i], totals[i] = T, expected[i] = E, *n_found their number
 *              (DEVICE pointers in _dev).  n <= SMATRIX_POPULAR_MAX.  The host flavour zero-fills the unused entries; _dev leaves them.
 * Returns -1, outputs as they were and the device untouched, for n == 0 or n > SMATRIX_POPULAR_MAX; base NULL, base == now or the two
 * matrices on different devices; num == 0, den == 0 or num > den; an unknown measure; shrink negative, NaN or infinite (-0.0 acts
 * as 0.0); deny_n > 2^32, or deny_bits NULL with deny_n != 0; any output pointer NULL.  0 otherwise, an empty `now` included
 * (n_found = 0).
 * How: smatrix_cf_popular's steps over 96-bit keys.  A key per slot of now's directory (one head-cell gather and ONE look-up of the
 * id in base's directory per row), a device-wide MSB radix select of up to 12 byte passes from the highest byte in which the keys
 * differ, the keys at or above the threshold collected with one atomic add per workgroup, one workgroup that sorts them in LDS
 * and looks T and E up again for the entries it stores.  _dev makes no read-back at all.  Scratch (now's read-path scratch): 12
 * bytes per slot of now's directory, 12 n bytes and a control block of 13 KiB.
 * Locks, mirrors, streams: BOTH matrix locks are held for the call, taken in address order (smatrix_merge's rule: this call and a
 * merge of the same two matrices cannot wait for each other); scalar writes still in either host mirror are written back first;
 * the scratch is ordered behind the previous read-path call on `now` whatever its stream.  hip_stream == NULL synchronises.  _dev
 * with a stream returns with its work enqueued: NEITHER matrix may be written or closed until the stream has passed that work.
 * Neither matrix is modified; file-backed matrices work unchanged.  Deterministic. */
enum { SMATRIX_TREND_GAIN = 0, SMATRIX_TREND_RATIO = 1, SMATRIX_TREND_ZSCORE = 2 };
int smatrix_cf_trending(smatrix_t* now, smatrix_t* base, int measure, uint32_t num, uint32_t den, double shrink,
                        const uint32_t* deny_bits, uint64_t deny_n, uint32_t min_total, uint32_t min_gain, uint32_t n,
                        uint32_t* ids, double* scores, uint32_t* totals, uint32_t* expected, uint32_t* n_found);
int smatrix_cf_trending_dev(smatrix_t* now, smatrix_t* base, int measure, uint32_t num, uint32_t den, double shrink,
                            const uint32_t* d_deny_bits, uint64_t deny_n, uint32_t min_total, uint32_t min_gain, uint32_t n,
                            uint32_t* d_ids, double* d_scores, uint32_t* d_totals, uint32_t* d_expected, uint32_t* d_n_found,
                            void* hip_stream);

/* k results for cold sessions: smatrix_cf_recommend_sim, then the free places of a short result filled from a list the caller
 * gives -- popular (smatrix_cf_popular), trending or editorial; the library does not care which -- under the session's own filters.
 * A new visitor, a session of long-tail items or one whose candidates are mostly excluded or denied still gets k results.
 *   scored     exactly smatrix_cf_recommend_sim with the same arguments: n_scored[s] is its counts[s], and the entries
 *              [s*k, s*k + n_scored[s]) of ids / scores are its bytes.  The same kernels are launched the same way; only what
 *              follows them is new.
 *   fill       when n_scored[s] < k, fill_ids[0 .. n_fill) is walked in list order and id f is appended with score +0.0 iff
 *              f != 0, f is not an item of the session at any position (repeats and items of weight 0 included), f is not on
 *              the session's exclusion list, f is not denied, and f is not in the session's result already, scored or filled
 *              earlier -- which also settles repeats inside the list.  The walk stops at k entries or at the list's end;
 *              counts[s] = n_scored[s] + the ids appended.  f needs no row in the matrix: the list is the caller's.  A filled id
 *              is never one of the session's candidates: with n_scored[s] < k every candidate left is in the result already.
 *   empty list fill_ids NULL with n_fill == 0: the call writes smatrix_cf_recommend_sim's bytes and n_scored = counts.
 *   unused     entries beyond counts[s]: the host flavour zero-fills them, _dev leaves them.
 * Cost beyond the sim call's: one launch, a wave per session.  A session with counts[s] == k ends after one load.  A session that
 * fills tests 64 list ids a step, a lane each: about (L + E + k + 64) compares per id walked (L the session's length, E its
 * exclusion list's), and at most k + L + E + (the zeros, denied ids and repeats in the list) ids are walked -- nothing for the short
 * sessions that need filling.  _dev adds no read-back; the host flavour stages fill_ids once and copies n_scored back.
 * Returns -1 for smatrix_cf_recommend_sim's refusals, word for word, and for n_scored NULL, fill_ids NULL with n_fill != 0 and
 * n_fill >= 2^32 (before the device is touched, outputs as they were).  0 otherwise. */
int smatrix_cf_recommend_fill(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                              const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                              const uint32_t* deny_bits, uint64_t deny_n, const uint32_t* fill_ids, uint64_t n_fill, int sim,
                              double shrink, uint32_t k, uint32_t* ids, double* scores, uint32_t* counts, uint32_t* n_scored);
int smatrix_cf_recommend_fill_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                  const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                  const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_fill_ids, uint64_t n_fill,
                                  int sim, double shrink, uint32_t k, uint32_t* d_ids, double* d_scores, uint32_t* d_counts,
                                  uint32_t* d_n_scored, void* hip_stream);

/* k results AND at most `cap` of one group: smatrix_cf_recommend_fill under caps.  smatrix_cf_recommend_grouped, then the free places
 * of a short result filled from the caller's list under the session's own filters and under the same quotas -- ten results, never
 * more than two of one brand, never fewer than ten.  Everything not said here is smatrix_cf_recommend_grouped's and
 * smatrix_cf_recommend_fill's contract, word for word: sessions, candidates, scores, filters, group_of / group_n / cap, fill_ids /
 * n_fill, tiers, locks, the mirror, streams, scratch, k <= 64.
 *   scored     exactly smatrix_cf_recommend_grouped with the same arguments: n_scored[s] is its counts[s], and the entries
 *              [s*k, s*k + n_scored[s]) of ids / scores are its bytes, through its own launches in both tiers.
 *   fill       when n_scored[s] < k, fill_ids[0 .. n_fill) is walked in list order and id f is appended with score +0.0 iff it
 *              passes every test of smatrix_cf_recommend_fill (f != 0, not an item of the session at any position, not on its
 *              exclusion list, not denied, not in the result already, scored or filled) AND f is ungrouped (f >= group_n or
 *              group_of[f] == SMATRIX_GROUP_NONE) or fewer than cap entries of the session's result so far, scored and filled
 *              together, have the group group_of[f].  An id refused by its quota does not end the walk, and a repeat of it is
 *              refused again; a repeat of an id that was taken is in the result already and consumes nothing.  The walk stops at
 *              k entries or at the list's end; counts[s] = n_scored[s] + the ids appended, which may still be < k.
 *   candidates left behind: under quotas n_scored[s] < k no longer means that the session's candidates are used up -- the ones the
 *              quota refused are still there.  Each of them belongs to a group that is full, and a full group stays full, so the
 *              fill's quota refuses it as well when the list offers it: a filled id is still never one of the session's candidates.
 *   no quota   a map that cannot bind (group_of NULL with group_n == 0, or cap >= k) makes the call smatrix_cf_recommend_fill: its
 *              bytes in all four outputs through its launches.
 *   empty list fill_ids NULL with n_fill == 0: smatrix_cf_recommend_grouped's bytes and n_scored = counts.
 *   unused     entries beyond counts[s]: the host flavour zero-fills them, _dev leaves them.
 * Deterministic: the same contents and input give the same bytes.
 * Cost beyond the grouped call's: the fill call's one launch, a wave per session; a session with counts[s] == k ends after one load.
 * A session that fills gathers one group per scored result once and one per list id that passed the fill's own tests, and decides
 * the quotas of 64 list ids at a time from two counts (the result's entries of the id's group, the step's earlier ids of it): 64
 * more compares per id walked than the fill call's.  Ids of full groups are walked past, 64 a step: a list dominated by one brand
 * costs its length / 64 steps.  The host flavour stages group_of and fill_ids once per call.
 * Returns -1 for smatrix_cf_recommend_grouped's refusals and smatrix_cf_recommend_fill's, word for word (both flavours before the
 * device is touched, outputs as they were; a bad weight as in the fill call: the host flavour before the device is touched, _dev on
 * the device, and nothing is filled behind it).  0 otherwise.
 * Not here: a cap per group, k > 64 (smatrix_cf_recommend_deep has neither list nor quotas), a fill list per session, and the sharded
 * matrix. */
int smatrix_cf_recommend_grouped_fill(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                                      const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                                      const uint32_t* deny_bits, uint64_t deny_n, const uint32_t* group_of, uint64_t group_n,
                                      uint32_t cap, const uint32_t* fill_ids, uint64_t n_fill, int sim, double shrink, uint32_t k,
                                      uint32_t* ids, double* scores, uint32_t* counts, uint32_t* n_scored);
int smatrix_cf_recommend_grouped_fill_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                          const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                          const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_group_of,
                                          uint64_t group_n, uint32_t cap, const uint32_t* d_fill_ids, uint64_t n_fill, int sim,
                                          double shrink, uint32_t k, uint32_t* d_ids, double* d_scores, uint32_t* d_counts,
                                          uint32_t* d_n_scored, void* hip_stream);

/* Recommendations from these categories only: smatrix_cf_recommend_grouped_fill with a scope per session -- a category page,
 * "accessories for this item", "more from this seller", a user's muted categories.  A scope is a per-session deny decided by the
 * candidate's group, applied on the GPU where a candidate is made, before the cut at k: a session whose best 64 candidates hold two
 * pairs of shoes still gets its 10 results for the shoe page.  The five arguments behind deny_n are new; everything not said here is
 * smatrix_cf_recommend_grouped_fill's contract, word for word, its special cases included (a map group_of that cannot bind makes it
 * the fill call, an empty fill list the grouped call, both together the sim call): one call covers a scope with any of filters,
 * measure, quotas and back-fill.  k <= 64.
 *   scope_of   one uint32 per id 0 .. scope_n - 1, scope_n <= 2^32: a second map, independent of group_of -- category here, brand
 *              there; the same array may be passed twice.  g(b) = scope_of[b] for b < scope_n, else SMATRIX_GROUP_NONE.
 *   sc_offsets, sc_groups   session s's scope list is sc_groups[sc_offsets[s] .. sc_offsets[s+1]): at most SMATRIX_SCOPE_MAX entries,
 *              repeats allowed, an entry SMATRIX_GROUP_NONE matches nothing.  sc_offsets has n_sessions + 1 entries and need not
 *              start at 0 (host flavour).
 *   listed(s, b)   g(b) != SMATRIX_GROUP_NONE and g(b) occurs in session s's list.
 *   unscoped   a session with an empty list is unscoped in both modes: every id is allowed.  One batch mixes scoped and unscoped
 *              sessions.
 *   scope_mode SMATRIX_SCOPE_ONLY: otherwise b is allowed iff listed(s, b); an ungrouped id is never given to a scoped session.
 *              SMATRIX_SCOPE_EXCEPT: otherwise b is allowed iff !listed(s, b); ungrouped ids pass.  One mode for the call.
 *   not allowed   an id that is not allowed is treated exactly as an id on the session's exclusion list: it is no candidate, consumes
 *              no quota, does not count in n_scored or counts, and the fill walks past it without ending the walk.  As an ITEM of
 *              the session it stays an item: its row is scanned and its weight counts.
 *   equivalence   the four outputs are the bytes of smatrix_cf_recommend_grouped_fill with the same arguments, when that call is given
 *              session s's exclusion list extended by every id that is not allowed for s.
 *   no scope   sc_offsets NULL (then sc_groups and scope_of must be NULL and scope_n 0) writes smatrix_cf_recommend_grouped_fill's
 *              bytes through that call's own launches.
 *   unused     entries beyond counts[s]: the host flavour zero-fills them, _dev leaves them.
 * Deterministic: the same contents and input give the same bytes; nothing depends on slot order, lane order or the tier.
 * Cost beyond the grouped fill call's: per DISTINCT candidate key of a scoped session (not per term) one 4-byte gather from scope_of
 * and at most SMATRIX_SCOPE_MAX compares against the session's list, read from global memory at an address the wave shares; per fill
 * step of 64 list ids one gather and 64 compares per id.  An unscoped session of a scoped batch pays one length test per key.  The
 * host flavour stages scope_of once per call and the lists as it stages the exclusion lists.
 * Returns -1 for smatrix_cf_recommend_grouped_fill's refusals, word for word, and for an unknown scope_mode, scope_n > 2^32, scope_of
 * NULL with scope_n != 0, exactly one of sc_offsets / sc_groups NULL, a map given without lists (all before the device is touched,
 * outputs as they were, both flavours), and for a list longer than SMATRIX_SCOPE_MAX, found as a bad weight is found: the host
 * flavour walks sc_offsets before the device is touched, _dev finds it on the device, leaves the outputs unspecified, and nothing
 * is filled behind it.  0 otherwise.
 * Not here: k > 64, smatrix_cf_rank / smatrix_cf_explain under a scope, a mode per session, and the sharded matrix. */
#define SMATRIX_SCOPE_MAX 64
enum { SMATRIX_SCOPE_ONLY = 0, SMATRIX_SCOPE_EXCEPT = 1 };
int smatrix_cf_recommend_scoped(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* items,
                                const double* weights, const uint64_t* ex_offsets, const uint32_t* ex_items,
                                const uint32_t* deny_bits, uint64_t deny_n, const uint32_t* scope_of, uint64_t scope_n,
                                const uint64_t* sc_offsets, const uint32_t* sc_groups, int scope_mode, const uint32_t* group_of,
                                uint64_t group_n, uint32_t cap, const uint32_t* fill_ids, uint64_t n_fill, int sim, double shrink,
                                uint32_t k, uint32_t* ids, double* scores, uint32_t* counts, uint32_t* n_scored);
int smatrix_cf_recommend_scoped_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_items,
                                    const double* d_weights, const uint64_t* d_ex_offsets, const uint32_t* d_ex_items,
                                    const uint32_t* d_deny_bits, uint64_t deny_n, const uint32_t* d_scope_of, uint64_t scope_n,
                                    const uint64_t* d_sc_offsets, const uint32_t* d_sc_groups, int scope_mode,
                                    const uint32_t* d_group_of, uint64_t group_n, uint32_t cap, const uint32_t* d_fill_ids,
                                    uint64_t n_fill, int sim, double shrink, uint32_t k, uint32_t* d_ids, double* d_scores,
                                    uint32_t* d_counts, uint32_t* d_n_scored, void* hip_stream);

/* CF-recommender write path, on the device (examples/cf_recommender.c:36-47 import_preference_set): session s is
 * ids[offsets[s] .. offsets[s+1]); for every position n of a session  incr(ids[n], 0, 1)  and, for every OTHER position i,
 * incr(ids[n], ids[i], 1) -- L*L ops for a session of L ids, generated on the GPU and applied as incr batches (the
 * batch contract above: any order, same final state).  offsets has n_sessions+1 entries.
 * _dev: all arrays in device memory; d_op_offsets[s] = sum of L*L over the sessions before s (n_sessions+1 entries),
 * total_ops = its last entry. */
int smatrix_cf_import_sessions(smatrix_t* self, size_t n_sessions, const uint64_t* offsets, const uint32_t* ids);
int smatrix_cf_import_sessions_dev(smatrix_t* self, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_ids,
                                   const uint64_t* d_op_offsets, uint64_t total_ops, void* hip_stream);

/* The write path with a window, amounts and a way back: what a session MEANS to the matrix is chosen by the caller, and a
 * session that was imported can be taken out again.  Session s is the positions p = 0 .. L-1 of ids[offsets[s] .. offsets[s+1])
 * (n_sessions + 1 non-decreasing offsets); its amounts are w_p = amounts[offsets[s] + p], or 1 everywhere with amounts NULL.
 * The call applies, each exactly once:
 *   head op    for every position p with w_p != 0:  op(id_p, 0, w_p).
 *   pair op    for every ordered pair of positions (p, q), p != q, with w_p != 0 and w_q != 0:  op(id_p, id_q, min(w_p, w_q)),
 *              provided that ALL of
 *                window == 0 (no limit) or |p - q| <= window.  Distances are counted in positions; a position of amount 0 still
 *                    occupies its place;
 *                with SMATRIX_IMPORT_FORWARD, q > p: row a then holds what came AFTER a ("what came next").  Without the flag
 *                    both directions are applied;
 *                with SMATRIX_IMPORT_NO_SELF, id_p != id_q.  Without it an id that occurs twice counts against itself, as in
 *                    smatrix_cf_import_sessions.
 *   why min    the pair amount is min(w_p, w_q): it keeps the matrix symmetric without FORWARD, and with distinct ids it keeps
 *              cc(a, b) <= min(total(a), total(b)), so the read path's guard cc > den -> 0 never fires on honest data.  A pair
 *              amount of w_q alone would score a view-then-buy pair 0.
 *   op         SMATRIX_OP_INCR or SMATRIX_OP_DECR.  A DECR of what an earlier INCR call with the same arguments applied restores
 *              every value exactly (uint32, wrapping, as the reference's smatrix_decr); the cells and rows stay, as dead cells
 *              (a pruning merge, min_value 1, removes them).  A DECR of what was never imported wraps.  A DECR call applies
 *              all its pair ops first and its head ops after them, in internal batches of their own: a head cell that reaches
 *              0 is the empty slot (quirk Q3) and cuts the probe chains of its row, so it has to be the LAST thing that happens
 *              to a row that is forgotten altogether -- every cell of such a row then stays where it is, with the value 0.
 *   id 0       is not special-cased, as in smatrix_cf_import_sessions.
 * With (SMATRIX_OP_INCR, amounts NULL, window 0, flags 0) these are exactly the ops of smatrix_cf_import_sessions, and *n_ops is
 *   the sum of L * L.  That call stays as it is; it is not routed through this one.
 * Result: the batch contract at the top of this file for the whole call as if it were ONE batch: values are exact, row sizes and
 *   `used` are the reference's.  The result does not depend on max_batch in anything the contract fixes.
 * Bounded scratch: the ops are generated on the device and applied in internal batches of at most max_batch ops -- max_batch ==
 *   0: 2^25; above 2^31: 2^31.  Device memory taken beyond the matrix is proportional to that bound plus 8 bytes per session
 *   (and 8 per 2048 sessions), never to the number of ops.  The per-session op offsets the generator needs are made by the
 *   library, on the device, with a scan over the sessions: _dev takes none and no total.  The generator walks a slot space of
 *   L * min(L, 2 * window + 1) slots per session (FORWARD: L * min(L, window + 1); window 0: L * L) and compacts the slots that
 *   are ops within each batch, so a batch may hold fewer than max_batch ops; one that holds none is not applied.
 * *n_ops (a HOST pointer in both flavours, may be NULL) receives the number of ops applied.
 * Returns -1 with nothing changed and *n_ops untouched for: an op other than INCR / DECR, unknown flag bits, n_sessions >= 2^32,
 *   offsets that decrease, a slot space of 2^63 slots or more.  The host flavour finds the last two on the host, _dev on the
 *   device before the first write (one 8-byte read-back).  0 otherwise, n_sessions == 0 included.
 * Locks, mirror, files, streams are smatrix_cf_import_sessions_dev's: the matrix lock for the call; scalar writes still in the
 *   host mirror are written back first and the mirror is dropped; column-0 adds are the single 64-bit add (no result array);
 *   smatrix_stats_t::batches counts the internal batches, and a call during which SMATRIX_FLUSH_EVERY falls due takes ONE
 *   checkpoint, at its end; file-backed matrices work unchanged.  The host flavour runs on the matrix's own stream and returns
 *   when done.  _dev: arrays in device memory on the matrix's GPU, work on hip_stream, complete on it when the call returns
 *   (NULL = the legacy default stream, synchronised before returning). */
enum { SMATRIX_IMPORT_FORWARD = 1, SMATRIX_IMPORT_NO_SELF = 2 };   /* flags, may be or-ed */
int smatrix_cf_import_events(smatrix_t* self, int op, size_t n_sessions, const uint64_t* offsets, const uint32_t* ids,
                             const uint32_t* amounts, uint32_t window, uint32_t flags, uint64_t max_batch, uint64_t* n_ops);
int smatrix_cf_import_events_dev(smatrix_t* self, int op, size_t n_sessions, const uint64_t* d_offsets, const uint32_t* d_ids,
                                 const uint32_t* d_amounts, uint32_t window, uint32_t flags, uint64_t max_batch,
                                 uint64_t* n_ops, void* hip_stream);

/* ---- whole-matrix export ------------------------------------------------- */
enum { SMATRIX_EXPORT_TABLE = 0, SMATRIX_EXPORT_SORTED = 1 };

/* Every row of the matrix and every pair its getrow would return, as CSR:
 *   rows[i]                      row id, i < n_rows
 *   row_ptr[i] .. row_ptr[i+1]   its pairs, at pairs + 2*row_ptr[i] (uint32 units; {column, value}, the getrow_batch layout)
 * TABLE:  rows in directory-slot order; each row's pairs in table-slot order, byte-identical to smatrix_getrow_batch of that
 *         row with an unlimited buffer.  Deterministic for a given table state.
 * SORTED: rows ascending by id, pairs ascending by column.  Depends only on the matrix's contents, not on its history.
 * Row set = the ids x for which smatrix_row_info(x) returns 1: a row with no pairs (quirk Q3, set(x,0,0) on a new row) is
 * listed with row_ptr[i] == row_ptr[i+1].  A row's pair count is its number of non-empty slots, NOT rowlen (quirks Q1/Q5).
 * row_ptr == NULL: size query -- writes *n_rows, *nnz, returns 0.
 * Returns 0 when written; 1 when n_rows > cap_rows or nnz > cap_nnz (nothing written, *n_rows / *nnz = what is needed);
 * -1 for an unknown order.  row_ptr must hold cap_rows + 1 entries.  n_rows / nnz are HOST pointers in both flavours.
 * Both take the matrix lock for their whole run; scalar writes still held in the host mirror are written back first.
 * _dev: buffers in device memory on the matrix's GPU, work on hip_stream (NULL = the legacy default stream); the call returns
 * after the export has completed on that stream (it reads the sizes back). */
int smatrix_export(smatrix_t* self, int order, uint64_t cap_rows, uint64_t cap_nnz,
                   uint32_t* rows, uint64_t* row_ptr, uint32_t* pairs, uint64_t* n_rows, uint64_t* nnz);
int smatrix_export_dev(smatrix_t* self, int order, uint64_t cap_rows, uint64_t cap_nnz,
                       uint32_t* d_rows, uint64_t* d_row_ptr, uint32_t* d_pairs,
                       uint64_t* n_rows, uint64_t* nnz, void* hip_stream);

/* ---- merge of two matrices, CSR import ------------------------------------- */
/* smatrix_merge:       dst[x,y]  op=  src[x,y]  for every pair of src; op is SMATRIX_OP_SET, _INCR or _DECR
 *                      (total += part; a sliding window: total += today, total -= day_30).
 * smatrix_import_csr:  the same with the pairs taken from a CSR in smatrix_export's layout (rows[n_rows], row_ptr[n_rows + 1],
 *                      pairs = {column, value} interleaved): the inverse of smatrix_export.
 * Which ops: merge applies op(x, y, v) once for every pair (y, v) that smatrix_export(src, TABLE) lists under row x -- every
 *   non-empty slot, value-0 cells with a non-zero key included (an incr by 0 creates the cell, as in the reference).  A source
 *   row without pairs (quirk Q3) contributes nothing and is not created in dst.  import_csr applies one op per pair of the CSR;
 *   a row id may occur more than once in rows, and a column more than once in a row.
 * Result: the batch contract at the top of this file for the whole call as if it were ONE batch: the final state is what the
 *   reference reaches by applying those ops one by one in some order; values are exact (uint32, wrapping); row sizes and `used`
 *   are the reference's.  SET with a key that occurs more than once in the CSR: the LAST occurrence (highest position in pairs)
 *   wins, also when the occurrences fall into different internal batches.  Nothing beyond the batch contract is promised for
 *   the layout of a row's table.
 * Bounded scratch: the work runs in internal batches of at most max(max_batch, longest source row) ops -- max_batch == 0: 2^24,
 *   the batch size the write path is tuned for; above 2^31: 2^31 -- (import_csr: of exactly max_batch pairs, rows are split).
 *   Device memory taken beyond the matrices is proportional to that bound plus 20 bytes per source ROW (import_csr host flavour:
 *   12 per row), never to the number of pairs: no whole-matrix CSR, no triples.  The result does not depend on max_batch in
 *   anything the contract fixes (values, row set, sizes, `used`).
 * *n_ops (may be NULL) receives the number of ops applied.  Returns 0; -1 and nothing changed for: an op other than SET / INCR /
 *   DECR, dst == src, the two matrices on different devices, a CSR whose row_ptr is not non-decreasing from 0 (checked on the
 *   device before the first write).
 * Locks and mirrors: merge holds both matrices' locks for the call, taken in one global order (merge(a, b) and merge(b, a) on
 *   two threads cannot deadlock); it takes no file lock, so the file-then-matrix order of smatrix_flush holds.  Scalar writes
 *   still in src's and dst's host mirrors are written back first (as smatrix_export does) and dst's mirror is dropped.
 *   File-backed dst and src work unchanged: the rows dst changed are DIRTY and reach its file by the usual flush;
 *   smatrix_stats_t::batches counts the internal batches, and a call during which SMATRIX_FLUSH_EVERY falls due takes ONE
 *   checkpoint, at its end.  src is not modified.
 * merge and the host flavour of import_csr run on the matrix's own stream and return when done.  _dev: arrays in device memory
 *   on the matrix's GPU, work ordered after hip_stream's earlier work and complete on it when the call returns (NULL = the
 *   legacy default stream). */
int smatrix_merge(smatrix_t* dst, smatrix_t* src, int op, uint64_t max_batch, uint64_t* n_ops);

/* smatrix_merge_scaled: smatrix_merge with a decay and a filter between src's row tables and the ops -- the call that ends a
 *   sliding-window cycle (total += today; total -= day_30; fresh = merge_scaled(empty, total, SET, 1, 1, 1): no dead cells, row
 *   tables of the size the survivors need) and the exponential forgetting of a CF recommender (num / den < 1).
 * Candidates: every pair (y, v) that smatrix_export(src, TABLE) lists under row x -- the pairs smatrix_merge applies.
 * Transform:  v' = floor(v * num / den), computed in 64 bits; 1 <= num <= den, so v' <= v and nothing overflows.
 * Filter:     a candidate is DROPPED when v' < min_value, or when y == 0 && v' == 0 (a (0, 0) cell is the empty slot, quirk Q3:
 *             it cannot be stored, and applying it would only cut probe chains).
 * Every other candidate is applied once as op(x, y, v'); op is SMATRIX_OP_SET, _INCR or _DECR.
 * *n_ops (may be NULL) receives the number of ops applied, *n_dropped (may be NULL) the number of candidates dropped; their
 *   sum is src's pair count.
 * So: num == den and min_value == 0 behaves as smatrix_merge (but for a (0, 0) pair, which the export never lists anyway).
 *   min_value == 1 drops every dead cell.  With min_value == 0 a (y != 0, 0) result still creates its cell (an incr by 0 does
 *   so in the reference).  A source row that loses all its pairs contributes nothing and is not created in dst.
 * Result: the batch contract at the top of this file for the whole call as if it were ONE batch: the final state is what the
 *   reference reaches by applying those ops one by one in some order; values are exact (uint32, wrapping); row sizes and `used`
 *   are the reference's -- into an empty dst, those of a matrix that never held the dropped pairs.  SET ties cannot occur:
 *   every key occurs once.  Nothing beyond the batch contract is promised for the layout of a row's table.
 * Bounded scratch: the work runs in internal batches of at most max(max_batch, longest SURVIVING row) ops -- max_batch == 0:
 *   2^24; above 2^31: 2^31.  Device memory taken beyond the matrices is proportional to that bound plus 20 bytes per source ROW
 *   (row list 8, survivor count 4, scan 8), never to the number of pairs.  The result does not depend on max_batch in anything
 *   the contract fixes (values, row set, sizes, `used`).
 * Returns 0; -1 and nothing changed for: an op other than SET / INCR / DECR, dst == src, the two matrices on different devices,
 *   den == 0, num == 0, num > den.
 * Locks and mirrors: both matrices' locks are held for the call, taken in address order; no file lock is taken.  Scalar writes
 *   still in src's and dst's host mirrors are written back first and dst's mirror is dropped.  File-backed dst and src work
 *   unchanged; smatrix_stats_t::batches counts the internal batches, and a call during which SMATRIX_FLUSH_EVERY falls due
 *   takes ONE checkpoint, at its end.  src is not modified (its tables never shrink in place: build the pruned matrix, then
 *   close the old one).  Runs on dst's own stream and returns when done. */
int smatrix_merge_scaled(smatrix_t* dst, smatrix_t* src, int op, uint32_t num, uint32_t den, uint32_t min_value,
                         uint64_t max_batch, uint64_t* n_ops, uint64_t* n_dropped);

/* smatrix_merge_topk: smatrix_merge that keeps, of every row of src, only the m heaviest pairs -- the neighbourhood truncation of
 *   an item-kNN recommender (total += today; total -= day_30; serving = merge_topk(empty, total, SET, m, 1): every row of the
 *   serving copy holds at most m + 1 pairs, whatever the row held in total).
 * Candidates: every pair (y, v) that smatrix_export(src, TABLE) lists under row x -- the pairs smatrix_merge applies.
 * Head pair:  the pair with y == 0 (the CF example's per-item total) is kept iff v >= min_value && v != 0 (a (0, 0) cell is the
 *             empty slot, quirk Q3) and never counts against m: the kept pairs score in the copy as they do in src, and the
 *             cosine needs the totals of both items.
 * Eligible:   y != 0 && v >= min_value.  With min_value == 0 a dead cell (y != 0, v == 0) is eligible, ranks below every live
 *             pair and, when kept, creates its cell in dst as in smatrix_merge.
 * Rank:       key(y, v) = ((uint64_t)v << 32) | (0xFFFFFFFF - y), larger is better: by value, equal values by ascending column.
 *             Keys are unique within a row; the row keeps its min(m, eligible) eligible pairs of the largest keys.  The kept set
 *             depends on src's contents alone -- not on slot order, insertion history or max_batch.
 * Every kept pair is applied once as op(x, y, v); op is SMATRIX_OP_SET, _INCR or _DECR.  Everything else is dropped.
 * *n_ops (may be NULL) receives the number of ops applied, *n_dropped (may be NULL) the number of candidates dropped; their
 *   sum is src's pair count.  A source row that keeps nothing contributes nothing and is not created in dst.
 * Result: the batch contract at the top of this file for the whole call as if it were ONE batch: the final state is what the
 *   reference reaches by applying those ops one by one in some order; values are exact (uint32, wrapping); row sizes and `used`
 *   are the reference's -- into an empty dst, those of a matrix that never held the dropped pairs.  SET ties cannot occur:
 *   every key occurs once.  Nothing beyond the batch contract is promised for the layout of a row's table.
 * Bounded scratch: the work runs in internal batches of at most max(max_batch, longest SURVIVING row) ops -- max_batch == 0:
 *   2^24; above 2^31: 2^31.  Device memory taken beyond the matrices is proportional to that bound plus 28 bytes per source ROW
 *   (row list 8, kept count 4, scan 8, threshold 8), never to the number of pairs.  The result does not depend on max_batch in
 *   anything the contract fixes (values, row set, sizes, `used`).
 * Returns 0; -1 and nothing changed for: m == 0, an op other than SET / INCR / DECR, dst == src, the two matrices on different
 *   devices.
 * Locks and mirrors: both matrices' locks are held for the call, taken in address order; no file lock is taken.  Scalar writes
 *   still in src's and dst's host mirrors are written back first and dst's mirror is dropped.  File-backed dst and src work
 *   unchanged; smatrix_stats_t::batches counts the internal batches, and a call during which SMATRIX_FLUSH_EVERY falls due
 *   takes ONE checkpoint, at its end.  src is not modified (its tables never shrink in place: build the truncated matrix, then
 *   close the old one).  Runs on dst's own stream and returns when done. */
int smatrix_merge_topk(smatrix_t* dst, smatrix_t* src, int op, uint32_t m, uint32_t min_value, uint64_t max_batch,
                       uint64_t* n_ops, uint64_t* n_dropped);

/* smatrix_merge_topk_by: smatrix_merge_topk with the rank of a row's pairs chosen by the caller.  Everything not said here is
 *   smatrix_merge_topk's contract, word for word: candidates, head pair, eligibility, the op applied -- op(x, y, v) with the RAW
 *   v, so the copy scores its kept pairs as src does --, the counts, the batch contract, bounded scratch, locks, mirrors, files,
 *   the one checkpoint, src untouched.
 * rank == SMATRIX_RANK_VALUE:  smatrix_merge_topk itself (the same code path).
 * rank == SMATRIX_RANK_COSINE: the row keeps the pairs that SCORE best in the CF read path (smatrix_cf_neighbors, _topk,
 *   _recommend), not the heaviest ones: a popular item co-occurs with everything, has a large v and a small cosine, and under
 *   the value rank crowds an item's truly similar neighbours out of the kept m.
 *   total(i) = what smatrix_get(src, i, 0) returns once the mirror is written back; 0 without a row or a head pair.
 *   The score of the pair (y, v) of row x, in IEEE double, expression for expression that of smatrix_cf_neighbors:
 *       tb = total(y); if (tb == 0) tb = 1;
 *       den = sqrt((double)total(x)) * sqrt((double)tb);
 *       score = (den != 0.0 && !((double)v > den)) ? (double)v / den : 0.0;
 *   Rank key: the pair (bit pattern of score as uint64, 0xFFFFFFFF - y), compared lexicographically, larger is better: by
 *       score (scores are >= 0, so their bit patterns order as the doubles do), equal scores by ascending column.  Keys are
 *       unique within a row; the row keeps its min(m, eligible) eligible pairs of the largest keys.
 *   A row without a head pair scores 0 everywhere and keeps its m LOWEST eligible columns.  A dead cell (v == 0, eligible with
 *       min_value == 0) scores 0, as does a pair with v > den.
 *   The kept set depends on src's contents alone -- not on slot order, insertion history or max_batch.
 * Device memory beyond the matrices: smatrix_merge_topk's plus the column half of the threshold -- 32 bytes per source ROW
 *   (row list 8, kept count 4, scan 8, threshold 8 + 4) and nothing per pair: there is no per-pair score array, every pass
 *   over a row makes the scores it needs again.
 * Returns 0; -1 and nothing changed (n_ops and n_dropped untouched) for an unknown rank and for smatrix_merge_topk's refusals. */
enum { SMATRIX_RANK_VALUE = 0, SMATRIX_RANK_COSINE = 1 };
int smatrix_merge_topk_by(smatrix_t* dst, smatrix_t* src, int op, int rank, uint32_t m, uint32_t min_value,
                          uint64_t max_batch, uint64_t* n_ops, uint64_t* n_dropped);

/* smatrix_merge_topk_sim: smatrix_merge_topk_by(SMATRIX_RANK_COSINE) with the score of smatrix_cf_recommend_sim (above) in place of
 *   the cosine, so that a serving copy is cut by the score it will be read by:
 *   truncated by (sim, shrink), it answers smatrix_cf_recommend_sim(sim, shrink) for one-item sessions and k <= m as src does.
 *   Everything not said here is smatrix_merge_topk_by's contract for the cosine rank, word for word: candidates, head pair,
 *   eligibility, the rank key (bit pattern of the score, 0xFFFFFFFF - y: scores are >= 0, so the patterns order as the doubles
 *   do; equal scores by ascending column), the op applied with the RAW v, the counts, the batch contract, locks, mirrors, files,
 *   the one checkpoint, src untouched, and the 32 bytes of device memory per source ROW with nothing per pair.
 *   The score of the pair (y, v) of row x is smatrix_cf_recommend_sim's with a = x, b = y, cc = v.  A row without a head pair
 *   scores 0 everywhere and keeps its m LOWEST eligible columns; a dead cell scores 0, as does a pair with v > den.
 * sim == SMATRIX_SIM_COSINE with shrink == 0 is smatrix_merge_topk_by(SMATRIX_RANK_COSINE) itself (the same code path).
 * Returns 0; -1 and nothing changed (n_ops and n_dropped untouched) for an unknown sim, a shrink that is negative, NaN or
 *   infinite, and for smatrix_merge_topk's refusals.  smatrix_merge_topk_by knows the two ranks above and no other. */
int smatrix_merge_topk_sim(smatrix_t* dst, smatrix_t* src, int op, int sim, double shrink, uint32_t m, uint32_t min_value,
                           uint64_t max_batch, uint64_t* n_ops, uint64_t* n_dropped);
int smatrix_import_csr(smatrix_t* self, int op, uint64_t n_rows, const uint32_t* rows, const uint64_t* row_ptr,
                       const uint32_t* pairs, uint64_t max_batch, uint64_t* n_ops);
int smatrix_import_csr_dev(smatrix_t* self, int op, uint64_t n_rows, const uint32_t* d_rows,
                           const uint64_t* d_row_ptr, const uint32_t* d_pairs, uint64_t max_batch,
                           uint64_t* n_ops, void* hip_stream);

/* Capacity hint, like vector::reserve: map at least `bytes` of device memory for row tables now instead of in growth
 * steps later (each step is a call into the driver, normally ~0.3 ms, but one that can block for seconds while the driver
 * still has freed memory to wipe).  Nothing observable changes.  Returns 0. */
int smatrix_reserve(smatrix_t* self, uint64_t bytes);

/* smatrix_close keeps up to SMATRIX_CHUNK_POOL_GB (default 64, 0 = nothing) of the closed matrix's device memory for the
 * next matrix this process opens (memory handed back to the driver is wiped before reuse, and allocating into that wipe
 * blocks for seconds); this gives it back at once. */
void smatrix_release_cached_memory(void);

/* ---- introspection (tests, bench) ---------------------------------------- */
typedef struct {
  uint64_t rows;            /* rows in the directory */
  uint64_t dir_slots;       /* directory capacity */
  uint64_t arena_units;     /* 128-byte units handed out (incl. retired blocks) */
  uint64_t arena_mapped;    /* bytes of HBM mapped for row tables */
  uint64_t arena_free_units;/* units in retired blocks waiting for reuse */
  uint64_t batches;         /* write batches executed */
  uint64_t rounds;          /* op-kernel rounds over all write batches */
  uint64_t deferred_ops;    /* ops re-run after a structure change */
  uint64_t rows_grown;      /* row doublings */
  uint64_t dir_grown;       /* directory rebuilds */
  uint64_t rows_rebalanced; /* big rows whose insert quotas were re-partitioned */
  uint64_t long_probe_rounds; /* rounds in which ops were handed to the wave-cooperative window probe (clustered ids) */
  uint64_t scalar_cache_hits;    /* scalar-ABI calls answered from the host-side cell mirror (no device round trip) */
  uint64_t scalar_cache_flushes; /* write-backs of mirrored values (one batched set each) */
  uint64_t scalar_cache_flushed_cells;
  uint64_t bulk_rounds;          /* write batches whose deferred ops were grouped by row (the bulk path, k_fix_*) */
  uint64_t bulk_ops;             /* ops finished on that path */
  uint64_t file_flushes;         /* file mode: write-outs of dirty rows (smatrix_flush, SMATRIX_FLUSH_EVERY, close) */
  uint64_t file_rows_written;    /* rows those write-outs wrote (a clean row is never rewritten) */
  uint64_t file_leaked_bytes;    /* row blocks that grown rows left behind in the file since it was opened */
  uint64_t file_compactions;     /* smatrix_compact runs */
  uint64_t spec_chains;          /* write batches whose rounds 0 and 1 were enqueued at once, with one read-back (run_write) */
  uint64_t spec_refused;         /* of those: chains in which a growth task did not fit the estimates and was left to the host-driven loop */
  uint64_t file_bg_flushes;      /* of file_flushes: those the background flusher made (SMATRIX_FLUSH_MS, default 100; 0 = off) */
  uint64_t cold_starts;          /* write batches whose large remainder was reduced to its distinct keys before the rounds went on (insert_pending_keys) */
  uint64_t cold_keys;            /* distinct keys those inserted */
  uint64_t clustered_mode;       /* 1 once a write batch had >= 1/64 of its ops finished by the wave-cooperative probe (unscrambled ids: long runs
                                    under the reference's identity hash): large rows are then doubled in two passes, retry lists run a wave per op */
  uint64_t set_located_by_fold;  /* set batches that round 0 completed: their entries' cells were the ones k_set_fold had found (no locate pass) */
  uint64_t flush_snapshots_refused; /* flushes that could not get their snapshot buffer on the device and wrote under the matrix lock instead */
  /* profiling (smatrix_profile): HIP-event time, launches and ops of the round-0 op kernel,
   * indexed by op code (SMATRIX_OP_GET/SET/INCR/DECR) */
  double   kernel_ms[4];
  uint64_t kernel_launches[4];
  uint64_t kernel_ops[4];
  /* (round 6; new fields are APPENDED from here on -- see smatrix_stats_sz) what the write batches cost the calling thread:
   * wall time inside the write path, of it blocked on the device (read-backs between rounds: kernels were running), of it
   * inside device allocations / frees / address-range maps; call - wait - alloc is host work with the device idle or ahead.
   * Totals since open, then the same for the most recent write batch. */
  double   write_call_ms, write_wait_ms, write_alloc_ms;
  double   last_write_call_ms, last_write_wait_ms, last_write_alloc_ms;
} smatrix_stats_t;

void smatrix_stats(smatrix_t* self, smatrix_stats_t* out);
/* The same for callers that may have been compiled against an older (shorter) version of the struct: at most `size` bytes
 * are written (pass sizeof(smatrix_stats_t) as the caller's header defines it).  Fields are only ever appended. */
void smatrix_stats_sz(smatrix_t* self, smatrix_stats_t* out, size_t size);
/* File mode: writes every row that changed since the last flush to the backing file NOW (dirty rows only -- in
 * place when the row's table still has its on-disk size, else as a fresh block whose CMAP entry is re-pointed, the
 * reference's own scheme, src/smatrix.c:418-496); row blocks first, then the entries that publish them.  smatrix_close
 * does the same one last time.  The reference has no such call: its IO thread flushes continuously (:929-960) and
 * close is its only barrier (:113-133).  Like the reference's IO thread (100 ms poll, :945) a background flusher of this
 * library writes dirty rows every SMATRIX_FLUSH_MS milliseconds (default 100, 0 = off), so a process that dies without
 * close loses about that much.  Both -- this call and the background flusher -- hold the matrix lock only while the dirty
 * rows are collected, laid out and SNAPSHOT on the device (at most SMATRIX_FLUSH_SNAPSHOT_MB = 2048 MB of row tables at a
 * time; a larger backlog goes out in several such steps); the copies to the host and the writes run without it, as the
 * reference's IO thread writes under per-row read locks only (:929-960): callers on other threads keep their latency
 * (measured: a 1 GB flush, batch gets p99 23 -> 25 us).  A row that changes while a flush writes goes out with the next.
 * SMATRIX_FLUSH_EVERY=N checkpoints after every N-th write batch (by the call that made it, once it has released the matrix
 * lock; a host-pointer call that runs in chunks is ONE batch), SMATRIX_FSYNC=1 adds fsync() after the row blocks and after the
 * entries.  Memory mode: no-op.  Returns 0.
 * Lock order (round 6): the FILE lock first, then the matrix lock, everywhere -- smatrix_flush, the background flusher, a
 * SMATRIX_FLUSH_EVERY checkpoint, smatrix_compact, smatrix_close.  A flush keeps the file lock while it writes and holds the
 * matrix lock only for its snapshot; whoever wants the file next queues for it WITHOUT the matrix lock, so no caller of the
 * handle ever stands behind a thread that waits for a write in flight
 * (tests/test_gpu_round6.py::test_a_second_flush_does_not_hold_up_the_callers). */
int smatrix_flush(smatrix_t* self);
/* EXPERIMENTAL, no reference counterpart (the reference's files only grow: resized rows leave their old block behind,
 * src/smatrix.c:430-436, and so do this library's -- same format, same leak): rewrites the backing file without those
 * blocks, all rows into a new file next to it, fsync, rename over the old one.  Needs room for a second copy while it
 * runs.  SMATRIX_COMPACT_AT_CLOSE=1 does it at close.  Not part of the drop-in surface; may change.  Returns 0. */
#ifdef SMATRIX_EXPERIMENTAL
/* (only for callers that define SMATRIX_EXPERIMENTAL, and only active in a process run with SMATRIX_EXPERIMENTAL=1 in its
 *  environment: otherwise the call prints a note, leaves the file alone and returns -1) */
int smatrix_compact(smatrix_t* self);
#endif
/* on: time every round-0 op kernel with HIP events on its stream (adds one sync per
 * batch); resets the kernel_* accumulators. */
void smatrix_profile(smatrix_t* self, int on);
/* returns 1 if the row exists; size = slots, used = rowlen */
int smatrix_row_info(smatrix_t* self, uint32_t x, uint32_t* size, uint32_t* used);
/* copies the row's raw {key,value} slots (slot order); returns its size, 0 if absent */
uint32_t smatrix_row_slots(smatrix_t* self, uint32_t x, uint32_t* kv, uint32_t cap_slots);
/* 1 if a HIP device is usable; the library never falls back to a CPU path */
int smatrix_device_available(void);

#ifdef __cplusplus
}
#endif
#endif
