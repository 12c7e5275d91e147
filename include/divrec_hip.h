/*
 * libdivrec_hip — C ABI of the MI355X (gfx950) hot path of divrec
 * (amtsyplov/diversity-recommendations). Plain pointers and sizes only; no
 * torch types. Every pointer argument is DEVICE memory owned by the caller
 * unless the comment says otherwise. The library never allocates device
 * memory: scratch comes from a caller-owned workspace sized by the matching
 * *_workspace() query. All work is enqueued asynchronously on `stream`
 * (a hipStream_t; NULL = the legacy default stream).
 *
 * Return value: DR_OK (0) or a negative DR_E* code; dr_last_error() then holds
 * a thread-local message. The Python host (divrec/_backend.py) raises
 * RuntimeError(dr_last_error()) on any non-zero status.
 *
 * Reference entry points each function replaces are cited as
 * path:line relative to the reference tree (divrec/ ...).
 */
#ifndef DIVREC_HIP_H_
#define DIVREC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dr_stream_t; /* hipStream_t */

enum dr_status {
  DR_OK = 0,
  DR_EINVAL = -1,       /* bad shape / pointer / argument */
  DR_EUNSUPPORTED = -2, /* unsupported d / k / dtype combination */
  DR_EHIP = -3,         /* HIP runtime error (launch failure etc.) */
  DR_EWORKSPACE = -4    /* workspace too small */
};

enum dr_dtype { DR_F32 = 0, DR_BF16 = 1, DR_I32 = 2, DR_I64 = 3, DR_F64 = 4 };

enum dr_ild_kind {
  DR_ILD_COSINE = 0,    /* 1 - <e_i,e_j> / (|e_i| |e_j|) */
  DR_ILD_DOT = 1,       /* <e_i,e_j> */
  DR_ILD_EUCLIDEAN = 2  /* |e_i - e_j|_2 */
};

/* Library version (major*10000 + minor*100 + patch). */
int dr_version(void);
/* Build id: the first 16 hex digits of a sha256 over the library's source files
 * (the .hip and .h files of csrc/ and include/), baked in at compile time, so a run can
 * show which sources the loaded library was built from. */
const char* dr_build_id(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* dr_last_error(void);

/* Planner knobs: process-wide overrides of dr_score_topk's launch planner (and
 * of dr_mmr_rerank's, dr_dpp_rerank's, dr_calibrated_rerank's and
 * dr_xquad_rerank's grids, DR_KNOB_SCAN_SLOTS), for tests and A/B timing runs
 * only. Every plan gives identical results; only the time differs. The
 * library reads no environment variable: a knob holds the default plan until
 * it is set here, and value NaN restores the default. Thread-safe (atomic). */
enum dr_plan_knob {
  DR_KNOB_SCAN_SLOTS = 0,   /* workgroup slots planned for (split-tail plans at small sizes) */
  DR_KNOB_SCAN_SPLIT = 1,   /* max catalog chunks of a tail block (1 = no split) */
  DR_KNOB_TAIL_KEYS = 2,    /* finalize key cap of a split-tail user */
  DR_KNOB_SCAN_SEED = 3,    /* 0: never seed from a sample; 1: always (>= 2^18 rows) */
  DR_KNOB_GUESS_STRIDE = 4, /* sample stride of the guessed thresholds */
  DR_KNOB_GUESS_Z1 = 5,     /* set: ks1 = mu + z sigma + c1 instead of the 0.5 % Poisson-tail rank */
  DR_KNOB_GUESS_C1 = 6,     /* set: the offset c1 of that form (z defaults to 3) */
  DR_KNOB_GUESS_TIGHT = 7,  /* 0: one tier (ks1 = ks) */
  DR_KNOB_SAMPLE_DENSE = 8, /* 0: sample scan on compacted key buffers, not dense tile maxima; >1: budget GiB */
  DR_KNOB_ILD_STREAM = 9,   /* dr_ild_embedding, k <= 128: 0 = one wave per user, 1 = streamed persistent grid (default: streamed for d = 128 cosine / dot, k > 40) */
  DR_KNOB_ILD_BUFS = 10,    /* streamed ILD: ring slots (1-KB row pieces) per wave, at least one list's (default: as many as LDS allows) */
  DR_KNOB_SCAN_FLOOR = 11,  /* rows of the shortest graded tail chunk of dr_score_topk's seeded main scan (default 2^16; a value >= items / chunks: equal chunks) */
  DR_KNOB_SCAN_QUEUE = 12,  /* 0: the seeded main scan runs the static unit loop on equal tail chunks (no device unit queue) */
  DR_KNOB_COUNT = 13
};
/* Set knob `knob` to `value` (NaN = default). DR_EINVAL for an unknown knob,
 * an infinite value or one outside the knob's range: SCAN_SLOTS, SCAN_SPLIT,
 * TAIL_KEYS and GUESS_STRIDE take integers in [1, 2^30]; SCAN_SEED, GUESS_TIGHT
 * and ILD_STREAM 0 or 1; GUESS_Z1 / GUESS_C1 any finite value in [-64, 64];
 * SAMPLE_DENSE 0 (off), 1 (on, the default budget) or a budget in GiB above
 * 1 (up to 2^20); ILD_BUFS an
 * integer in [1, 64]; SCAN_FLOOR an integer in [32, 2^30] (one item tile at
 * the least); SCAN_QUEUE 0 or 1. */
int dr_set_plan_knob(int knob, double value);
/* Current value of a knob (NaN = default; NaN for an unknown knob). */
double dr_get_plan_knob(int knob);

/* ---------------------------------------------------------------------------
 * Id range checks (all gather-type calls below): an id outside [0, rows) of
 * its table — what nn.Embedding / tensor indexing reject with IndexError in
 * the reference — is never dereferenced. The affected unit (pair, triple,
 * user) produces NaN / adds nothing, and *err (caller-zeroed int32, may be
 * NULL) is incremented once per such unit. The host raises IndexError when
 * it reads a non-zero count.
 *
 * MatrixFactorization.forward: s[n] = sum_d U[user_id[n], d] * I[item_id[n], d]
 * Replaces divrec/models/matrix_factorization.py:26-28 (two nn.Embedding
 * lookups + torch.sum(u * i, dim=1)). Tables row-major [rows, d], dtype
 * DR_F32 or DR_BF16 (both tables the same dtype); ids int64; out fp32 [n].
 * Runs of equal ids (RankingDataset's full((n,), u), PairWiseDataset's m x m
 * pairs, divrec/datasets/base_datasets.py:94-107,165-171) read each row once.
 */
int dr_gather_dot(const void* user_table, int64_t n_user_rows, const void* item_table,
                  int64_t n_item_rows, int dtype, int64_t d, const int64_t* user_id,
                  const int64_t* item_id, int64_t n, float* out, int32_t* err,
                  dr_stream_t stream);

/* Backward of dr_gather_dot into DENSE fp32 gradient tables (nn.Embedding with
 * sparse=False, divrec/models/matrix_factorization.py:16-17):
 *   grad_user[user_id[n]] += grad_out[n] * I[item_id[n]]
 *   grad_item[item_id[n]] += grad_out[n] * U[user_id[n]]
 * Accumulates with fp32 atomics (order-dependent in the last bits). Either
 * grad pointer may be NULL to skip that table. Tables must be DR_F32. */
int dr_gather_dot_backward(const float* user_table, int64_t n_user_rows, const float* item_table,
                           int64_t n_item_rows, int64_t d, const int64_t* user_id,
                           const int64_t* item_id, int64_t n, const float* grad_out,
                           float* grad_user, float* grad_item, int32_t* err, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Full-catalog scoring + top-K: for each of the n_users user rows, the k best
 * items of the catalog slice [item_base, item_base + n_items) by
 * score = <U[user], I[item]>. Replaces get_model_recommendations
 * (divrec/train/utils.py:53-77) over RankingDataset candidates
 * (divrec/datasets/base_datasets.py:136-171), which scores each candidate with
 * MatrixFactorization.forward (divrec/models/matrix_factorization.py:26-28).
 *
 * Ranking order is score descending, item id ascending (the deterministic
 * tie-break the reference's unstable argsort leaves undefined, utils.py:73).
 *
 *   dtype       DR_BF16: bf16 tables, bf16 MFMA (exact products, fp32 sums) —
 *               the fast mode; d in {32, 64, 128, 256, 512}.
 *               DR_F32: fp32 tables, fp32 MFMA (an exact fp32 fmaf chain per
 *               score, the reference's own arithmetic up to summation order) —
 *               the faithful mode; d in {32, 64, 128, 256}.
 *               Other widths: pad both tables with zero columns (exact).
 *   user_table  [*, d]; user_ids int64 [n_users] or NULL (rows 0..n_users-1)
 *   item_table  [n_items, d] (the rows of THIS slice; global id = item_base + row)
 *   1 <= k <= 1024
 *   excl_rowptr int64 [n_users + 1], excl_items int32 (GLOBAL item ids, sorted
 *     ascending per row): items excluded per user (RankingDataset `frozen`,
 *     base_datasets.py:143-149). Both NULL = no exclusion.
 *   out_scores fp32 [n_users, k], out_items int32 [n_users, k] (GLOBAL ids);
 *     slots with no candidate hold item -1 and score -inf.
 *   workspace of dr_score_topk_workspace(...) bytes (query with identical args,
 *     with the device that runs the call current: the launch plan, and with it
 *     the size, depends on the device's CU count). Its size: candidate buffers
 *     of n_users (rounded up to a user block) x CAP x 8 B (CAP 512, 1024 or
 *     2048 by d and k), plus rows for the extra chunks of a split tail; for
 *     catalogs of 2^18 rows or more (the guessed thresholds) that region is
 *     instead the sample scan's dense [users x sample tiles] fp32 tile-max
 *     matrix when that is larger and within the SAMPLE_DENSE budget (16 GiB by
 *     default; 1M x 10M at d = 128: 9.8 GB against 8.5 GB of buffers), plus
 *     about 40 B per user of thresholds and fail lists and a copy of the
 *     sample rows.
 */
size_t dr_score_topk_workspace(int64_t n_users, int64_t n_items, int dtype, int d, int k);
int dr_score_topk(const void* user_table, const int64_t* user_ids, int64_t n_users,
                  const void* item_table, int64_t n_items, int64_t item_base, int dtype, int d,
                  int k, const int64_t* excl_rowptr, const int32_t* excl_items,
                  float* out_scores, int32_t* out_items, void* workspace,
                  size_t workspace_bytes, dr_stream_t stream);

/* The launch plan dr_score_topk uses for these arguments on the current device
 * (host-only query, no device work; the planner knobs of dr_set_plan_knob
 * included), so tests can show which plan they exercised. out[0..11] = users per
 * workgroup, user blocks, head blocks (scanned whole), catalog chunks per tail
 * block (1 = no split), tail chunk length, grid, candidate capacity, sample
 * stride of the guessed threshold (0 = plain scan), sample rows, sample rank ks,
 * finalize keys of a head user, finalize keys of a tail user; with n_out >= 13,
 * out[12] = the first-tier rank ks1 <= ks the main scan starts from. n_out >= 12. */
int dr_score_topk_plan(int64_t n_users, int64_t n_items, int dtype, int d, int k, int64_t* out,
                       int n_out);

/* The catalog chunks the main scan of dr_score_topk gives each tail block for
 * these arguments (host-only query, knobs included): *n_chunks = c (out[3] of
 * dr_score_topk_plan) and bounds[0..c] (host int64), chunk j = rows
 * [bounds[j], bounds[j + 1]). Where the scan's workgroups claim their units
 * from a device queue (the seeded main scan) the chunks are graded, longest
 * first; else they are equal. n_bounds > c (17 always suffices).
 * dr_tail_chunk_bounds is the rule itself: c chunks of whole stages of
 * stage_items rows (whole 32-row tiles) over n_items < 2^31 rows, halving from
 * the first until a chunk would fall below floor_items (in [1, 2^31)), the
 * rest equal; floor_items >= n_items / c gives c equal chunks. c in [1, 16]. */
int dr_score_topk_tail_chunks(int64_t n_users, int64_t n_items, int dtype, int d, int k,
                              int64_t* bounds, int n_bounds, int* n_chunks);
int dr_tail_chunk_bounds(int64_t n_items, int chunks, int stage_items, int64_t floor_items,
                         int64_t* bounds);

/* Guess statistics of the last dr_score_topk call on `workspace` with these
 * arguments (host query; synchronises with a copy): out[0] = users whose
 * first-tier guessed threshold failed (rescanned from their safe threshold),
 * out[1] = users every guess failed (rescanned from -inf). 0, 0 for plain
 * scans (catalogs below 2^18 rows). int32 out[2] is HOST memory. */
int dr_score_topk_fail_counts(const void* workspace, int64_t n_users, int64_t n_items, int dtype,
                              int d, int k, int32_t* out);

/* The guessed thresholds of the item-sharded multi-GPU top-k, computed like
 * dr_score_topk's own guess: sample_rows [n_sample, d] (dtype as the user
 * table) are the whole catalog's rows at the guess stride, gathered from every
 * shard; the whole 32-row tiles of them (n_sample rounded down) are scanned by
 * the tile-max sample scan, and thr1[u] / thr2[u] (fp32 [n_users], device)
 * are set strictly below the ks1-th / ks-th best tile-max score of user u
 * (-inf when there are fewer): lower bounds of the user's ks1-th / ks-th best
 * sample score, the first-tier and safe thresholds of
 * divrec.distributed.thresholded_exchange (replaces nothing in the reference:
 * the scale-out of divrec/train/utils.py:53-77). 1 <= ks1 <= ks <= 256.
 * Workspace of dr_sample_thresholds_workspace(...) bytes. */
size_t dr_sample_thresholds_workspace(int64_t n_users, int64_t n_sample, int dtype, int d, int ks);
int dr_sample_thresholds(const void* user_table, const int64_t* user_ids, int64_t n_users,
                         const void* sample_rows, int64_t n_sample, int dtype, int d, int ks1,
                         int ks, float* thr1, float* thr2, void* workspace, size_t workspace_bytes,
                         dr_stream_t stream);

/* dr_score_topk with caller-given per-user thresholds: the top-k (same order)
 * of the items whose score is STRICTLY above init_thr[u]; slots past the last
 * such item hold item -1 and score -inf. init_thr fp32 [n_users] (-inf = plain
 * top-k). The item-sharded multi-GPU top-k passes thresholds guessed from a
 * sample of the whole catalog, so each shard returns only items that can
 * reach the global top-k (divrec.distributed.sharded_score_topk; replaces the
 * per-shard share of divrec/train/utils.py:53-77). Other arguments as
 * dr_score_topk; workspace of dr_score_topk_seeded_workspace(...) bytes.
 */
size_t dr_score_topk_seeded_workspace(int64_t n_users, int64_t n_items, int dtype, int d, int k);
int dr_score_topk_seeded(const void* user_table, const int64_t* user_ids, int64_t n_users,
                         const void* item_table, int64_t n_items, int64_t item_base, int dtype,
                         int d, int k, const float* init_thr, const int64_t* excl_rowptr,
                         const int32_t* excl_items, float* out_scores, int32_t* out_items,
                         void* workspace, size_t workspace_bytes, dr_stream_t stream);

/* Merge `parts` per-user top-k lists (each sorted by the order above) into one:
 *   in_scores/in_items [parts, n_users, k_in] -> out [n_users, k_out], k_out <= parts*k_in
 *   (k_out <= 1024 when parts*k_in > 2048; entries with item -1 are empty).
 * This is the exchange step of the item-row-sharded top-K:
 * shard partials are exchanged over RCCL and merged here; the result is
 * bit-identical to the single-device dr_score_topk over the whole catalog. */
int dr_topk_merge(const float* in_scores, const int32_t* in_items, int parts, int64_t n_users,
                  int k_in, int k_out, float* out_scores, int32_t* out_items,
                  dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Intra-list diversity, IntraListDiversityScore.recommendations_loss with
 * reduction 'none' (divrec/losses/intra_list_diversity_score.py:20-42):
 *   out[u] = (sum_{p<q} D[r[u,p], r[u,q]]) / (k * (k - 1))     (k = 1 -> NaN)
 * `recs` [n_users, k] item ids of dtype rec_dtype (DR_I32 or DR_I64); a list
 * holding an id outside [0, n_items) gives NaN and counts in *err (above).
 */

/* Dense distance matrix D [n_items, n_items] (dtype DR_F32, DR_F64, DR_I32 or
 * DR_I64). Float D is accumulated in its own precision in itertools.combinations order, like the
 * reference's Python sum (bit-exact); integer D is summed exactly. */
int dr_ild_dense(const void* recs, int rec_dtype, int64_t n_users, int k, const void* dist,
                 int dist_dtype, int64_t n_items, float* out, int32_t* err, dr_stream_t stream);

/* The un-normalised pair sum of the same lists, sum_{p<q} D[r[u,p], r[u,q]], the
 * reference's IntraListDiversityScore.user_ild (:36-42): accumulated in D's
 * own precision in combinations order (fp32 D: the Python sum of 0-d fp32
 * tensors, bit-exact; integer D: exact), stored as double (k = 1: 0). */
int dr_ild_dense_pair_sum(const void* recs, int rec_dtype, int64_t n_users, int k,
                          const void* dist, int dist_dtype, int64_t n_items, double* out,
                          int32_t* err, dr_stream_t stream);

/* Label equality D[i,j] = (label[i] == label[j]), the matrix of
 * IntraListBinaryUnfairnessScore.get_distance_matrix (:60-63), computed on the
 * fly from labels int64 [n_items] (exact integer count). Any k: lists of up to
 * 1024 stage their labels in LDS, longer ones read them through the cache. */
int dr_ild_labels(const void* recs, int rec_dtype, int64_t n_users, int k,
                  const int64_t* labels, int64_t n_items, float* out, int32_t* err,
                  dr_stream_t stream);

/* Distance computed on the fly from an item embedding table (bf16 [n_items, d],
 * d in {32, 64, 128, 256}, 1 <= k <= 16384) by bf16 MFMA Gram tiles per user
 * (kind: enum dr_ild_kind). k <= 128: the list in registers, fp32 accumulation;
 * longer lists (the reference's user_ild takes any length): the row tiles
 * streamed through the cache, tile sums accumulated in double. */
int dr_ild_embedding(const void* recs, int rec_dtype, int64_t n_users, int k,
                     const void* item_table, int64_t n_items, int d, int kind, float* out,
                     int32_t* err, dr_stream_t stream);

/* Gradient of the embedding ILD with respect to the item table: for every
 * list u and position p, ADDS to grad_item[r[u,p], :] the derivative of
 * scale * grad_out[u] * ILD_u, ILD_u = (sum_{p<q} D(e_p, e_q)) / (k (k - 1)),
 * with respect to row r[u,p]. With w = scale * grad_out[u] / (k (k - 1)),
 * e_p = item_table[r[u,p]] and sums over POSITIONS (a repeated item is two
 * positions of one row, as in the forward):
 *   dot:        row p += w (S - e_p),  S = sum_q e_q
 *   cosine:     n_p = |e_p|, u_p = e_p / n_p, t_p = (sum_q u_q) - u_p;
 *               row p += -w (t_p - (u_p . t_p) u_p) / n_p
 *               (a position whose row has zero norm gets no gradient and does
 *               not enter the sum; no NaN or Inf reaches grad_item)
 *   euclidean:  row p += w sum_{q != p, |e_p - e_q| > 0} (e_p - e_q) / |e_p - e_q|
 *               (pairs at distance exactly 0, a repeated item among them, add
 *               nothing; the distance is formed from the differences)
 * item_table is the fp32 [n_items, d] master table (not the forward's bf16
 * copy), 1 <= d <= 256 (any d); grad_item fp32 of the same shape, owned and
 * zeroed by the caller, accumulated with atomics; grad_out fp32 [n_users], NULL
 * = all ones. 1 <= k <= 128 (k = 1 adds nothing); n_users = 0 is a no-op. A
 * list holding an id outside [0, n_items) adds nothing for any of its
 * positions and counts once in *err (id range checks, above). */
int dr_ild_embedding_backward(const void* recs, int rec_dtype, int64_t n_users, int k,
                              const float* item_table, int64_t n_items, int d, int kind,
                              const float* grad_out, float scale, float* grad_item,
                              int32_t* err, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * BPR step (pair_wise_train_loop, divrec/train/utils.py:144-152, with
 * LogSigmoidDifferenceLoss, divrec/losses/log_sigmoid_difference_loss.py:11-14):
 *   x[b] = <U[u_b], I[p_b]> - <U[u_b], I[n_b]>
 *   loss[b] = -logsigmoid(x[b]);  hit[b] = (x_pos >= x_neg) (AUCScore, auc_score.py:6-10)
 *   g = -sigmoid(-x) * grad_scale  (grad_scale = 1/B for the 'mean' reduction)
 *   grad_user[u] += g (I[p] - I[n]); grad_item[p] += g U[u]; grad_item[n] -= g U[u]
 * fp32 tables [*, d]; ids int64 [B]; loss fp32 [B] and hit int32 [B] may be
 * NULL. Gradients are DENSE fp32 tables accumulated with atomics. A triple
 * with an out-of-range id adds nothing, gets loss NaN / hit 0 and counts in
 * *err (id range checks, above). */
int dr_bpr_fwd_bwd(const float* user_table, int64_t n_user_rows, const float* item_table,
                   int64_t n_item_rows, int64_t d, const int64_t* user_id,
                   const int64_t* pos_id, const int64_t* neg_id, int64_t batch,
                   float grad_scale, float* loss, int32_t* hit, float* grad_user,
                   float* grad_item, int32_t* err, dr_stream_t stream);

/* Point-wise MSE step (point_wise_train_loop, divrec/train/utils.py:108-115,
 * with MSELoss, divrec/losses/mse_loss.py:6-10):
 *   pred[b] = <U[u_b], I[i_b]>;  e = target[b] - pred[b];  loss[b] = e * e
 *   g = -2 e * grad_scale  (grad_scale = 1/B for the 'mean' reduction, 1 for 'sum')
 *   grad_user[u] += g I[i]; grad_item[i] += g U[u]
 * fp32 tables [*, d], d in [1, 512]; ids int64 [B]; target fp32 [B]; pred and
 * loss fp32 [B] may each be NULL. Gradients are DENSE fp32 tables accumulated
 * with atomics; either may be NULL, and with both NULL the call is
 * forward-only (no atomics: point_wise_score_loop, utils.py:19-24). A pair
 * with an out-of-range id adds nothing, gets pred / loss NaN and counts in
 * *err (id range checks, above). batch = 0 is a no-op. */
int dr_mse_fwd_bwd(const float* user_table, int64_t n_user_rows, const float* item_table,
                   int64_t n_item_rows, int64_t d, const int64_t* user_id,
                   const int64_t* item_id, const float* target, int64_t batch,
                   float grad_scale, float* pred, float* loss, float* grad_user,
                   float* grad_item, int32_t* err, dr_stream_t stream);

/* WARP step (Weston, Bengio, Usunier 2011, as LightFM implements it; not in
 * the reference). For pair b = (u, p), with s_p = <U[u], I[p]> in fp32:
 *   for trial t = 0 .. max_trials-1, in this order:
 *     c = draw(seed, pair_base + b, 0, t) % n_item_rows   (the counter-based hash
 *         of dr_sample_pairwise; dr_warp_candidates writes the same stream)
 *     c == p, c in u's positives row or c in u's exclusion row: the trial is
 *         used up, nothing is scored (LightFM counts such draws too)
 *     otherwise s_n = <U[u], I[c]>; s_n > s_p - margin (fp32): c is the
 *         violator, trials[b] = t + 1, the loop ends
 *   with a violator: L = log(max(1, (n_item_rows - 1) / trials)), the division
 *     in integers; loss[b] = L (margin - s_p + s_n), the hinge of this one
 *     triple evaluated in float64 (the test above is the fp32 one); neg_id[b] = c;
 *     g = L * grad_scale  (grad_scale = 1/B for the 'mean' reduction)
 *     grad_user[u] += g (I[c] - I[p]); grad_item[p] -= g U[u]; grad_item[c] += g U[u]
 *   without one: loss[b] = 0, neg_id[b] = -1, trials[b] = max_trials, no gradient.
 * The result is defined by trial order alone: it depends on no launch
 * geometry, and calls on parts of a batch with pair_base = the part's offset
 * give the whole call's neg_id and trials.
 * fp32 tables [*, d], d in [1, 512]; ids int64 [B]; the positives and the
 * exclusions as CSR over the user rows (rowptr int64 [n_user_rows + 1], items
 * int32 sorted per row), each CSR both pointers or both NULL; max_trials in
 * [1, 4096]; margin finite; pair_base >= 0; n_item_rows < 2^31 - 1. loss fp32
 * [B], neg_id int64 [B] and trials int32 [B] may each be NULL. Gradients are
 * DENSE fp32 tables accumulated with atomics; either may be NULL. A pair with
 * an out-of-range id reads and adds nothing, gets loss NaN / neg_id -1 /
 * trials 0 and counts in *err (id range checks, above). batch = 0 is a no-op. */
int dr_warp_fwd_bwd(const float* user_table, int64_t n_user_rows, const float* item_table,
                    int64_t n_item_rows, int64_t d, const int64_t* user_id,
                    const int64_t* pos_id, int64_t batch, const int64_t* pos_rowptr,
                    const int32_t* pos_items, const int64_t* excl_rowptr,
                    const int32_t* excl_items, int max_trials, float margin, uint64_t seed,
                    int64_t pair_base, float grad_scale, float* loss, int64_t* neg_id,
                    int32_t* trials, float* grad_user, float* grad_item, int32_t* err,
                    dr_stream_t stream);

/* The candidate stream of dr_warp_fwd_bwd, on the HOST (no HIP call):
 * out[b * max_trials + t] = draw(seed, pair_base + b, 0, t) % n_items for
 * b < n_pairs, t < max_trials, int32 in host memory. 1 <= n_items < 2^31 - 1.
 * For tests and baselines that restate the step outside the kernel. */
int dr_warp_candidates(uint64_t seed, int64_t pair_base, int64_t n_pairs, int max_trials,
                       int64_t n_items, int32_t* out);

/* Candidate rows dr_warp_fwd_bwd keeps in flight per round after a pair's
 * first in this build (a compile-time choice that changes no result;
 * DESIGN.md §3.6c). */
int dr_warp_round(void);

/* Dense Adam step in fp32 over n elements, the update torch.optim.Adam
 * (amsgrad=False, maximize=False) applies at divrec/train/utils.py:151:
 *   g = grad + weight_decay * param; m = lerp(m, g, 1 - beta1);
 *   v = beta2 * v + (1 - beta2) * g * g;
 *   param -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * `step` is the 1-based step count AFTER incrementing. Hyper-parameters are
 * doubles (Python floats); they are combined in double and cast to fp32 once,
 * as torch does. */
int dr_adam_dense(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  int64_t n, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int64_t step, dr_stream_t stream);

/* Row-sparse ("lazy") Adam, SURVEY.md §8f rank 3: the update
 * torch.optim.SparseAdam applies (torch/optim/_functional.py, sparse_adam) to
 * a coalesced sparse gradient with indices `rows` (unique, int64, [n_rows]) and
 * values grad[rows] read from a DENSE fp32 gradient table [*, d] (as
 * accumulated by dr_bpr_fwd_bwd). Only the listed rows of param / exp_avg /
 * exp_avg_sq change. zero_grad != 0 also zeroes grad[rows], leaving the table
 * all-zero for the next batch without a full memset. The reference trains with
 * dense Adam (divrec/train/utils.py:151 over sparse=False embeddings,
 * divrec/models/matrix_factorization.py:16-17); this is the opt-in alternative.
 * `step` is SparseAdam's state step AFTER incrementing. */
int dr_adam_rows(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t d,
                 const int64_t* rows, int64_t n_rows, double lr, double beta1, double beta2,
                 double eps, int64_t step, int zero_grad, dr_stream_t stream);

/* Device-side pairwise sampling, SURVEY.md §8f rank 4: the sampling of
 * PairWiseDataset.__iter__ (divrec/datasets/base_datasets.py:70-107) for the
 * users `users` [n_users] (int64 row ids), in that order:
 *   pos_out[b, :] = m draws with replacement, uniform over the user's unique
 *                   positives (CSR pos_rowptr [*+1] / pos_items int32, sorted);
 *   neg_out[b, :] = m draws with replacement, uniform over
 *                   [0, n_items) - positives - frozen (CSR excl_*, may be NULL),
 *                   by rejection (at most 4096 tries per draw);
 *   uid/pid/nid [n_users*m*m] int64 (optional, all or none): the m x m
 *                   Cartesian product, positive-major, as the reference yields it.
 * Draws come from a counter-based hash of (seed, user id, draw, try) instead of
 * Python's random stream: parity is distributional. *err_count (caller-zeroed)
 * counts failed draws: users without positives (the reference raises
 * IndexError) and negatives with an empty allowed set; their ids are -1. */
int dr_sample_pairwise(const int64_t* users, int64_t n_users, const int64_t* pos_rowptr,
                       const int32_t* pos_items, const int64_t* excl_rowptr,
                       const int32_t* excl_items, int64_t n_items, int m, uint64_t seed,
                       int32_t* pos_out, int32_t* neg_out, int64_t* uid, int64_t* pid,
                       int64_t* nid, int32_t* err_count, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Accuracy metrics of top-k lists against test interactions, per user
 * (SURVEY.md §8f rank 1): precision@k (divrec/metrics/precision_at_k.py:6-22),
 * recall@k (recall_at_k.py:6-22), AP@k with the reference's formula
 * sum_p cumhits(p)/(p+1) / k (average_precision_at_k.py:6-24) and NDCG@k
 * (normalized_discounted_cumulative_gain.py:6-23). Positives as CSR: rowptr
 * int64 [n_users+1], items int32 sorted per row. Any output may be NULL.
 * recall is NaN for a user without positives (the reference divides by 0). */
int dr_rank_metrics(const void* recs, int rec_dtype, int64_t n_users, int k,
                    const int64_t* pos_rowptr, const int32_t* pos_items, float* precision,
                    float* recall, float* avg_precision, float* ndcg, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Catalog histogram of recommendation lists: ADDS, for
 * every entry of recs [n_users, k] with 0 <= item < n_items, 1 to counts[item]
 * (int32 [n_items]) and its 0-based position to pos_sum[item] (uint64
 * [n_items], may be NULL). The caller zeroes both. Replaces the counting of
 * EntropyDiversityScore (divrec/metrics/entropy_diversity_score.py:19-26,
 * torch.unique counts) and PRI's avg_rank
 * (divrec/metrics/popularity_rank_correlation_for_items.py:28-39). Exact. */
int dr_catalog_histogram(const void* recs, int rec_dtype, int64_t n_users, int k,
                         int64_t n_items, int32_t* counts, uint64_t* pos_sum,
                         dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * MMR diversity re-rank (config 5; no reference symbol — SURVEY.md §8a a16):
 * per user, greedily pick k_out of the C candidates maximising
 *   lambda * score_i - (1 - lambda) * max_{j in S} cos(e_i, e_j)
 * (ties -> lowest candidate position; the max term is 0 before the first
 * pick). cand_items int32 [n_users, C], cand_scores fp32 [n_users, C] (-inf and
 * NaN count as -FLT_MAX), item_table bf16 [*, d]; out int32 [n_users, k_out]
 * (item ids in selection order). C <= 1024, k_out <= C, d in {64, 128}.
 * A row whose fp32 sum of squares is 0 has cosine 0 with every row, itself
 * included, and stays eligible on its score. +inf scores and non-finite item
 * rows are outside the contract.
 * Candidate ids < 0 are empty slots; ids >= n_items are added to *err (int32
 * device counter, may be NULL) and never picked. A user left without live
 * candidates gets -1 for the remaining picks. n_items = 0 is DR_EINVAL.
 * Launch: one workgroup per CU looping over the users (the next user's
 * candidates are prefetched while one runs). */
int dr_mmr_rerank(const int32_t* cand_items, const float* cand_scores, int64_t n_users, int C,
                  const void* item_table, int64_t n_items, int d, int k_out, float lambda,
                  int32_t* out_items, int32_t* err, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * DPP diversity re-rank (greedy MAP of a determinantal point process, Chen,
 * Zhang, Zhou, NeurIPS 2018; no reference symbol, as for MMR): per user,
 * greedily pick k_out of the C candidates maximising
 *   lambda * score_i + (1 - lambda) * logf(r_i)
 * over the live candidates with r_i > DR_DPP_EPS (ties -> lowest candidate
 * position). x_i is the unit-normalised row of candidate i, S = <x_i, x_j> the
 * cosine Gram matrix, and r_i = det S_{Y+i} / det S_Y = 1 - |P_Y x_i|^2 the
 * residual of i given the picked set Y (the Schur complement of the
 * incremental Cholesky of S). r_i starts at exactly 1.0f, so lambda = 0 makes
 * the first pick a tie that position 0 wins. After pick j every candidate
 * gets e_i = <b_t, x_i>, r_i -= e_i^2, b_t the t-th Gram-Schmidt vector of the
 * picked rows (= (S_ji - sum_t' c_t'j c_t'i) / sqrt(r_j) of the Cholesky form).
 * cand_items int32 [n_users, C], cand_scores fp32 [n_users, C], item_table
 * bf16 [*, d]; out_items int32 [n_users, k_out] (item ids in selection order),
 * out_resid fp32 [n_users, k_out] (may be NULL): r of each pick at the moment
 * it was picked, so sum log(out_resid) is the list's log det S.
 * 1 <= C <= 1024, 1 <= k_out <= min(C, 128), d in {64, 128}.
 * Never eligible: r_i <= DR_DPP_EPS (duplicates of a pick, dependent rows: fp32
 * leaves them at 0 +- 1e-6), candidate ids < 0 (empty slots), zero-norm rows;
 * ids >= n_items are added to *err (int32 device counter, may be NULL) and
 * never picked, their rows never read. When no eligible candidate is left
 * (rank exhausted, k_out > d, all duplicates) the remaining picks are -1 with
 * out_resid 0. n_items = 0 is DR_EINVAL.
 * Launch: one workgroup per CU looping over the users (DR_KNOB_SCAN_SLOTS caps
 * the grid, as for dr_mmr_rerank). */
#define DR_DPP_EPS 1e-4f
int dr_dpp_rerank(const int32_t* cand_items, const float* cand_scores, int64_t n_users, int C,
                  const void* item_table, int64_t n_items, int d, int k_out, float lambda,
                  int32_t* out_items, float* out_resid, int32_t* err, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Calibrated re-rank over item partition labels (Steck, "Calibrated
 * Recommendations", RecSys 2018; no reference symbol, as for MMR and DPP; the
 * labels are the reference's item_features["partition"], the surface of
 * IntraListBinaryUnfairnessScore, intra_list_diversity_score.py:45-63). Per
 * user: a profile row w[G] (fp32), normalised to p_g = max(w_g, 0) / sum_g
 * max(w_g, 0) (NaN counts as 0; a row whose sum is 0 gives p = 0, so every KL
 * below is 0; weights must be finite), labels l(i) in [0, G), and after t
 * picks the label counts n_g. For a candidate of label c
 *   q~_g(c) = (1 - alpha) (n_g + [g = c]) / (t + 1) + alpha p_g
 *   KL_c    = sum_{g : p_g > 0} p_g log(p_g / q~_g(c))     (finite: q~_g >= alpha p_g)
 *   value_i = lambda * score_i - (1 - lambda) * KL_{l(i)}
 * and each step picks the live candidate of highest value (ties -> lowest
 * candidate position), then n_{l(pick)} += 1. lambda = 1, G = 1 and a zero
 * profile row each give the stable order by score. cand_items int32
 * [n_users, C], cand_scores fp32 [n_users, C] (-inf and NaN count as -FLT_MAX),
 * item_labels int32 [n_items], profile fp32 [n_users, G]; out_items int32
 * [n_users, k_out] (item ids in selection order), out_kl fp32 [n_users, k_out]
 * (may be NULL): KL(p || q~) of the list after each pick.
 * Never live, never picked: candidate ids < 0 (empty slots); ids >= n_items
 * (added to *err, an int32 device counter that may be NULL; their label is
 * never read); candidates whose label is outside [0, G) (added to *err).
 * Positions are picked once each; duplicate ids are not detected. When no live
 * candidate is left the remaining picks are -1 and out_kl repeats the KL of
 * the list as it stands (-log(alpha) [sum p > 0] for an empty list), so
 * out_kl[:, k_out - 1] is the finished list's dr_calibration_kl.
 * 1 <= C <= 1024 and 1 <= G <= DR_CALIB_MAX_LABELS (above: DR_EUNSUPPORTED),
 * 1 <= k_out <= C, lambda in [0, 1]; n_items = 0 is DR_EINVAL.
 * Launch: one wave per user (lane g = category g, 16 candidates per lane),
 * four users per workgroup, a persistent grid (DR_KNOB_SCAN_SLOTS caps it, as
 * for dr_mmr_rerank). */
#define DR_CALIB_ALPHA 0.01f
#define DR_CALIB_MAX_LABELS 64
int dr_calibrated_rerank(const int32_t* cand_items, const float* cand_scores, int64_t n_users,
                         int C, const int32_t* item_labels, int64_t n_items, int G,
                         const float* profile, int k_out, float lambda, int32_t* out_items,
                         float* out_kl, int32_t* err, dr_stream_t stream);

/* Profiles for dr_calibrated_rerank from a history CSR (rowptr int64
 * [n_rows + 1], items int32; the exclusion CSR of dr_score_topk is one):
 * out[r, g] = (items of row r with label g) / (items of row r with a valid
 * label), fp32 [n_rows, G]; an empty row is a zero row. Items outside
 * [0, n_items) and labels outside [0, G) are skipped and counted in *err.
 * The counts are exact integers (rows of fewer than 2^24 items) and the value
 * is one fp32 divide of the two. Limits of G and n_items as above. */
int dr_label_profile(const int64_t* rowptr, const int32_t* items, int64_t n_rows,
                     const int32_t* item_labels, int64_t n_items, int G, float* out, int32_t* err,
                     dr_stream_t stream);

/* Calibration of finished lists: out[u] = KL(p || q~), q~_g = (1 - alpha) q_g +
 * alpha p_g, q_g the share of label g among the valid entries of recs[u, :]
 * ([n_users, k], rec_dtype DR_I32 or DR_I64) and p the normalised profile row,
 * as above. Entries < 0 (a list that ended early) are skipped; entries >=
 * n_items or with a label outside [0, G) are skipped and counted in *err. A
 * list without a valid entry has q = 0: -log(alpha) [sum p > 0]. */
int dr_calibration_kl(const void* recs, int rec_dtype, int64_t n_users, int k,
                      const int32_t* item_labels, int64_t n_items, int G, const float* profile,
                      float* out, int32_t* err, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * xQuAD aspect-aware re-rank over a multi-hot item-aspect matrix (Santos,
 * Macdonald, Ounis, "Exploiting Query Reformulations for Web Search Result
 * Diversification", WWW 2010; for recommendation: Vargas & Castells, RecSys
 * 2011; no reference symbol, as for MMR, DPP and the calibrated re-rank; the
 * aspects are columns of the reference's item_features, e.g. the 19 genre
 * columns of its ML-100K loader). item_aspects fp32 [n_items, G], row-major;
 * per user a profile row w[G] (fp32). With
 *   c_{i,a} = min(max(item_aspects[i, a], 0), 1)         (NaN counts as 0)
 *   p_a     = max(w_a, 0) / sum_a max(w_a, 0)            (NaN counts as 0; a row
 *             whose sum is 0 gives p = 0: the rules of dr_calibrated_rerank)
 * the uncovered mass m_a starts at p_a, and each step picks the live candidate
 * of highest
 *   value_i = lambda * score_i + (1 - lambda) * sum_a m_a c_{i,a}
 * (ties -> lowest candidate position), then m_a <- m_a (1 - c_{pick,a}).
 * lambda weights RELEVANCE, as in every re-ranker here; the paper's lambda is
 * 1 - lambda. lambda = 1, a zero profile row and an all-zero aspect matrix
 * each give the stable order by score exactly (the diversity term is +-0).
 * cand_items int32 [n_users, C] (ids < 0: empty slots), cand_scores fp32
 * [n_users, C] (-inf and NaN count as -FLT_MAX), profile fp32 [n_users, G];
 * out_items int32 [n_users, k_out] in pick order; out_cov fp32 [n_users,
 * k_out] (may be NULL): the list's coverage after each pick,
 *   sum_a (p_a - m_a) = sum_a p_a (1 - prod_{j in list} (1 - c_{j,a})),
 * accumulated from the steps' gains, which telescope: out_cov[:, k_out - 1] is
 * the finished list's dr_aspect_coverage.
 * Never live, never picked: ids < 0; ids >= n_items (added to *err, an int32
 * device counter that may be NULL; their row is never read). When no live
 * candidate is left the remaining picks are -1 and out_cov repeats. Positions
 * are picked once each; duplicate ids are not detected.
 * 1 <= C <= 1024 and 1 <= G <= DR_XQUAD_MAX_ASPECTS, and C * G <=
 * DR_XQUAD_MAX_CELLS: 128 KiB of fp32, the largest user block that leaves room
 * beside it in a CU's 160 KiB of LDS (beyond either: DR_EUNSUPPORTED);
 * 1 <= k_out <= C, lambda in [0, 1]; n_items = 0 with users present is
 * DR_EINVAL.
 * Arithmetic (fp32, no fused multiply-add): div_i = sum_a p_a c_{i,a} is summed
 * once in aspect order; a step forms value_i = lambda s_i + (1 - lambda) div_i,
 * and for each aspect of the pick with c_{pick,a} != 0, in aspect order:
 * delta = m_a c_{pick,a}, m_a -= delta, div_i -= delta c_{i,a}, cov += delta.
 * Launch: one 256-thread workgroup per user at a time with the user's clamped
 * C x G block aspect-major in LDS, a persistent grid of as many workgroups per
 * CU as are resident (DR_KNOB_SCAN_SLOTS caps the CUs, as for dr_mmr_rerank). */
#define DR_XQUAD_MAX_ASPECTS 64
#define DR_XQUAD_MAX_CELLS 32768
int dr_xquad_rerank(const int32_t* cand_items, const float* cand_scores, int64_t n_users, int C,
                    const float* item_aspects, int64_t n_items, int G, const float* profile,
                    int k_out, float lambda, int32_t* out_items, float* out_cov, int32_t* err,
                    dr_stream_t stream);

/* Profiles for dr_xquad_rerank from a history CSR (rowptr int64 [n_rows + 1],
 * items int32; the exclusion CSR of dr_score_topk is one):
 *   out[r, a] = sum_{i in row r} c_{i,a} / sum_a sum_{i in row r} c_{i,a}
 * fp32 [n_rows, G]; an empty or all-zero row gives a zero row. Items outside
 * [0, n_items) are skipped and counted in *err. No atomics: each (row, aspect)
 * is summed in the row's order by fp32 adds, the denominator is one fixed
 * tree over the aspects, so the result is bitwise reproducible; for binary
 * matrices the sums are exact integers (rows of fewer than 2^24 items) and the
 * value is one fp32 divide. Limits of G and n_items as above. */
int dr_aspect_profile(const int64_t* rowptr, const int32_t* items, int64_t n_rows,
                      const float* item_aspects, int64_t n_items, int G, float* out, int32_t* err,
                      dr_stream_t stream);

/* Expected aspect coverage of finished lists (the objective of dr_xquad_rerank;
 * subtopic recall, Zhai et al., SIGIR 2003, when p is uniform and the aspects
 * binary): out[u] = sum_a p_a (1 - prod_{j in recs[u, :]} (1 - c_{j,a})), p the
 * normalised profile row as above; recs [n_users, k], rec_dtype DR_I32 or
 * DR_I64. Entries < 0 (a list that ended early) are skipped; entries >=
 * n_items are skipped and counted in *err. A list without a valid entry
 * scores 0. */
int dr_aspect_coverage(const void* recs, int rec_dtype, int64_t n_users, int k,
                       const float* item_aspects, int64_t n_items, int G, const float* profile,
                       float* out, int32_t* err, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Distance of list items from the user's own history through the item
 * embeddings (unexpectedness and serendipity, Kaminskas & Bridge, TiiS 2016;
 * no reference symbol):
 *   out[u, p] = reduce_{h in H_u, 0 <= h < n_items} (1 - cos(e_{r[u,p]}, e_h))
 * lists int32 [n_users, C] (finished lists or candidate lists), 1 <= C <= 1024;
 * item_table bf16 [n_items, d], d in {32, 64, 128, 256}; the history is a CSR
 * (hist_rowptr int64 [n_users + 1], hist_items int32, rows of any length; the
 * exclusion CSR of dr_score_topk is one; hist_items may be NULL when every row
 * is empty); reduce DR_HIST_MIN or DR_HIST_MEAN; out fp32 [n_users, C].
 * The cosine is the fp32 Gram accumulation of the bf16 rows times 1/|e| of
 * both rows, 1 - g (w_h w_c) in one fused multiply-add. A row whose fp32 sum
 * of squares is 0 has cosine 0 with every row, so its distance is 1
 * (dr_mmr_rerank's rule). History entries outside [0, n_items) are skipped and
 * counted in *err (int32 device counter, may be NULL); their rows are never
 * read. A user with no valid history entry gets 0 for every valid list id,
 * for both reductions. List ids < 0 are empty slots and get 0; list ids >=
 * n_items get NaN (also for a user without history) and are counted in *err,
 * their rows never read. MEAN divides the sum by the number of valid history
 * entries; the sum runs in fp32 within a 32-row history tile and in double
 * across tiles. MIN is exact in its inputs and independent of the order of
 * the history. Duplicate history entries count once each (MEAN) and change
 * nothing (MIN). No float atomics: the result is bitwise reproducible.
 * n_users = 0 is a no-op success; bad sizes (C, n_users, n_items outside
 * [0, 2^31), reduce) are DR_EINVAL and another d is DR_EUNSUPPORTED, both
 * before any HIP call; n_items = 0 with users present is DR_EINVAL.
 * Launch: a persistent grid (DR_KNOB_SCAN_SLOTS caps the CUs, as for
 * dr_mmr_rerank); one wave serves a user when C <= 128, a workgroup above;
 * one user's history is never split across workgroups. */
enum dr_hist_reduce { DR_HIST_MIN = 0, DR_HIST_MEAN = 1 };
int dr_history_distance(const int32_t* lists, int64_t n_users, int C, const void* item_table,
                        int64_t n_items, int d, const int64_t* hist_rowptr,
                        const int32_t* hist_items, int reduce, float* out, int32_t* err,
                        dr_stream_t stream);

/* Serendipity re-rank: per user the first k_out candidates in stable
 * descending order of
 *   value_i = lambda * score_i + (1 - lambda) * dist_i
 * (fp32, two multiplies and one add, no fused multiply-add; ties -> lowest
 * candidate position), dist_i the dr_history_distance of candidate i, computed
 * by the same device function: out_dist (fp32 [n_users, k_out], may be NULL),
 * the picks' distances, is bitwise what dr_history_distance returns for the
 * same inputs. There is no greedy loop: one register sort per user of the keys
 * (value, position). -inf and NaN scores count as -FLT_MAX; +inf scores are
 * outside the contract. out_items int32 [n_users, k_out]: item ids in that
 * order. Candidate ids < 0 are never live; ids >= n_items are never live and
 * are added to *err. With fewer than k_out live candidates the remaining picks
 * are -1 with out_dist 0. 1 <= k_out <= C <= 1024, lambda in [0, 1]; n_items
 * = 0 with users present is DR_EINVAL. lambda = 1, and a user without valid
 * history, each give the stable order by score exactly. The other arguments,
 * the error codes and the launch are dr_history_distance's. */
int dr_serendipity_rerank(const int32_t* cand_items, const float* cand_scores, int64_t n_users,
                          int C, const void* item_table, int64_t n_items, int d,
                          const int64_t* hist_rowptr, const int32_t* hist_items, int reduce,
                          int k_out, float lambda, int32_t* out_items, float* out_dist,
                          int32_t* err, dr_stream_t stream);

/* Per-list mean of a per-item value (novelty: self-information or popularity
 * complement of the items): out[u] = mean of item_values[recs[u, p]] over the
 * valid entries of recs [n_users, k] (rec_dtype DR_I32 or DR_I64); item_values
 * fp32 [n_items]. Entries < 0 are skipped; entries >= n_items are skipped and
 * counted in *err. A list without a valid entry scores 0. The sum runs in
 * position order in fp32 and is divided once: reproducible. */
int dr_list_item_mean(const void* recs, int rec_dtype, int64_t n_users, int k,
                      const float* item_values, int64_t n_items, float* out, int32_t* err,
                      dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Implicit-feedback ALS row solve (Hu, Koren, Volinsky, ICDM 2008; no
 * reference symbol): one half-step of alternating least squares, and the
 * fold-in of rows the model has never seen. fixed_table Y fp32 [n_fixed_rows,
 * d] stays fixed; the rows to solve are a CSR over it (rowptr int64
 * [n_rows + 1], cols int32 [nnz], weights fp32 [nnz] or NULL = all 1). For
 * row r with entries (i, w_i):
 *   A_r = G + alpha * sum_i w_i y_i y_i^T + reg * I     G = Y^T Y, fp32 [d, d]
 *   b_r = sum_i (1 + alpha * w_i) y_i
 *   x_r = A_r^-1 b_r                                    (Cholesky, fp32)
 * the exact minimiser over x_r of sum_i c_ri (p_ri - x_r^T y_i)^2 + reg |x_r|^2
 * with c = 1 + alpha w, p = 1 on the row's entries and c = 1, p = 0 elsewhere.
 * gram is an argument (one d x d product per half-step, the caller's) and
 * must be symmetric. out fp32 [n_rows, d].
 * An empty row gives x_r = 0 exactly. A cols entry outside [0, n_fixed_rows)
 * contributes nothing and is added to *err (a 32-bit device counter, may be
 * NULL). A repeated column contributes once per occurrence. A row whose
 * Cholesky meets a pivot that is not finite or <= 0 (negative or non-finite
 * weights only) is a whole row of NaN. No atomics touch the result: a row
 * depends on its own entries only, bitwise, whatever the grid or its place in
 * the CSR. rowptr must be non-decreasing with rowptr[n_rows] = nnz (the
 * caller's to check; the kernel reads cols[rowptr[r] .. rowptr[r + 1])).
 * d in {32, 64, 128}, alpha >= 0, reg > 0 (all finite), n_fixed_rows in
 * [0, 2^31); cols may be NULL when every row is empty, fixed_table when
 * n_fixed_rows = 0. n_rows = 0 is a no-op.
 * Launch: one 256-thread workgroup per row at a time, a persistent grid of as
 * many workgroups per CU as are resident (DR_KNOB_SCAN_SLOTS caps the CUs, as
 * for dr_dpp_rerank). */
int dr_als_solve(const float* fixed_table, int64_t n_fixed_rows, int d, const float* gram,
                 const int64_t* rowptr, const int32_t* cols, const float* weights, int64_t n_rows,
                 float alpha, float reg, float* out, uint32_t* err, dr_stream_t stream);

/* ---------------------------------------------------------------------------
 * Weighted CSR row sum over an embedding table (no reference symbol): the
 * composition of a table from feature embeddings (a LightFM-style hybrid:
 * a row's embedding is the weighted sum of its features' embeddings) and,
 * over the transposed CSR, its exact gradient with respect to the feature
 * table. table fp32 [n_table_rows, d]; the rows to sum are a CSR over it
 * (rowptr int64 [n_rows + 1], cols int32 [nnz], weights fp32 [nnz] or NULL =
 * all 1):
 *   out[r, :] = sum_{e in [rowptr[r], rowptr[r + 1])} w[e] * table[cols[e], :]
 * out is [n_rows, d], out_dtype DR_F32 or DR_BF16; the bf16 form is the fp32
 * sum rounded once to nearest-even.
 * Order of the sum: a row's entries are cut into chunks of DR_ROW_SUM_CHUNK
 * (= L) consecutive entries; a chunk is summed from 0 in entry order by fp32
 * FMAs, and a row's chunk sums are added in chunk order. No atomics touch the
 * result: a row depends, bitwise, on its own entry list and on L only,
 * whatever the grid, the CU count, its place in the CSR, its neighbours, or
 * whether a plan is given.
 * The plan (optional; it decides who sums, never what): with plan = NULL, or
 * n_long = 0, the lane groups stride over the rows and one group sums a whole
 * row, however long. The plan of a CSR with rows longer than L lists EVERY
 * work item, longest first (a stable sort): each of a long row's chunks, whose
 * sum goes to a partial row of the workspace (fp32 [n_chunks, d],
 * dr_csr_row_sum_workspace bytes), and each other row whole. The groups take
 * the items in serpentine order, so their loads stay equal however skewed the
 * rows are, and a second kernel (one workgroup per long row) adds each long
 * row's partial rows in chunk order: a CSR with a few very long rows (the
 * transpose of a map with popular features) then costs about what an evenly
 * filled one does. With n_items = n_rows - n_long + n_chunks, plan is int64
 * [3 * n_items + 2 * n_long + 1] on the device, five lists one after the
 * other:
 *   item_row  [n_items]     the row of item i
 *   item_beg  [n_items]     its first entry, an index into cols: the item
 *                           covers at most L entries from there, to the
 *                           row's end at the latest
 *   item_slot [n_items]     the partial row its sum goes to, or -1: the item
 *                           is a whole row and goes to out
 *   long_row  [n_long]      the rows longer than L
 *   long_first[n_long + 1]  long row j owns the partial rows long_first[j] ..
 *                           long_first[j + 1], its chunks in order
 * A row that a given plan does not cover is not written (or not wholly
 * summed); an index outside its range is skipped, never followed: a wrong
 * plan gives wrong sums, never an access outside the arrays.
 * An empty row WRITES zeros. A cols entry outside [0, n_table_rows) adds
 * nothing and is added to *err (a 32-bit device counter, may be NULL). A
 * repeated column counts once per occurrence. rowptr must be non-decreasing
 * with rowptr[n_rows] = nnz (the caller's to check; the kernel reads
 * cols[rowptr[r] .. rowptr[r + 1])). 1 <= d <= DR_ROW_SUM_MAX_D,
 * n_table_rows in [0, 2^31), 0 <= 2 n_long <= n_chunks; cols may be NULL when
 * every row is empty, table when n_table_rows = 0. n_rows = 0 is a no-op.
 * Launch: lane groups of 4 .. 64 lanes, 16 B of a row per lane (d a multiple
 * of 4 and 16-B aligned pointers; one float per lane otherwise), several
 * entries' rows in flight per group; a persistent grid of as many 256-thread
 * workgroups per CU as are resident (DR_KNOB_SCAN_SLOTS caps the CUs, as for
 * dr_als_solve). No host synchronisation. */
#define DR_ROW_SUM_CHUNK 512
#define DR_ROW_SUM_MAX_D 512
int dr_csr_row_sum_chunk(void); /* DR_ROW_SUM_CHUNK of the built library */
size_t dr_csr_row_sum_workspace(int64_t n_chunks, int d);
int dr_csr_row_sum(const float* table, int64_t n_table_rows, int d, const int64_t* rowptr,
                   const int32_t* cols, const float* weights, int64_t n_rows,
                   const int64_t* plan, int64_t n_chunks, int64_t n_long, void* out,
                   int out_dtype, void* workspace, size_t workspace_bytes, uint32_t* err,
                   dr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIVREC_HIP_H_ */
