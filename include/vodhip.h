/*
 * vodhip.h -- C-ABI of the MI355X-native dense-retrieval scoring library (libvodhip.so).
 *
 * This is the drop-in boundary for the ONE hot path of VodLM/vod that this project replaces:
 * the corpus vector store + batched query x section inner-product top-k that the reference
 * reaches through a faiss server process, plus the hybrid score merge and the in-batch
 * retrieval scoring glued to it.  Plain pointers and sizes only; no torch / C++ types.
 * Reference citations are relative to /root/reference/.
 *
 * Conventions
 *   - every function returns 0 on success, < 0 on error; `vodhip_last_error()` returns a
 *     thread-local, NUL-terminated description of the last failure on the calling thread;
 *   - no exception crosses the boundary; the caller owns every buffer it passes in;
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the null stream).  Kernels are
 *     enqueued on it; functions documented "async" return before the GPU work is done;
 *   - device pointers must belong to the device the handle was created on;
 *   - result layout everywhere: scores float32 [nq,k] sorted descending, ids int64 [nq,k],
 *     ties -> smaller id first, missing entries padded with score -inf / id -1
 *     (the repo-wide padding convention, src/vod_types/retrieval.py:284-285).
 *     A VODHIP_L2 index returns squared L2 distances instead: sorted ASCENDING, ties -> smaller id, pads +inf / -1 (see VODHIP_L2).
 */
#ifndef VODHIP_H
#define VODHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VODHIP_VERSION 1

/* element types of vectors handed to / stored by the library */
enum { VODHIP_F16 = 0, VODHIP_BF16 = 1, VODHIP_F32 = 2 };
/* OR-ed into the store dtype at create: the store ALSO keeps the float32 rows and every search returns what a float32 brute force
 * over the unrounded rows and queries returns (H2 below) - the reference's own arithmetic: faiss IndexFlat holds float32
 * (`index.add(vectors.astype(float32))`, src/vod_search/faiss_search/build.py:65-73; float32 queries, faiss_search/server.py:71,81).
 * Costs 4 more bytes per element of HBM and ~1-3 % of search time.  Such a store takes dim <= 16384 (the float32 query sits in LDS
 * during re-scoring: 64 KB at the limit); vodhip_index_create refuses a wider one ("VODHIP_EXACT_F32 stores take dim <= 16384").
 * A plain store has no width limit of its own (tested up to dim 16384). */
#define VODHIP_EXACT_F32 0x100
/* OR-ed into the store dtype at create: the index ranks by SQUARED L2 DISTANCE (faiss.index_factory(D, "Flat", METRIC_L2): the
 * reference's FaissFactoryConfig.metric = "l2", src/vod_configs/search.py:21-27,143-149, faiss_search/build.py:60).
 * |q - x|^2 = |q|^2 - 2 (q.x - |x|^2 / 2): every row keeps c = -|x~|^2 / 2 behind its `dim` values, split into three store-dtype
 * terms; the queries are staged with three power-of-two constants behind theirs; the inner-product scan over dim + 3 columns then
 * searches L2 unchanged and one launch turns its scores into distances ("L2 metric").
 *   - the store keeps rows of dim + 3 columns, padded to a multiple of 64: vodhip_index_data's stride includes the bias columns;
 *     vodhip_index_dim, vodhip_index_get_rows and vodhip_index_add speak the user's `dim`;
 *   - SEARCH CONTRACT: out_scores are squared L2 distances of the stored (rounded) rows and the rounded queries, sorted ASCENDING,
 *     ties -> smaller id, clamped at 0; pads are (+inf, -1).  faiss pads L2 results with +FLT_MAX: a documented deviation, like the
 *     -inf pad of the inner-product side.  id_base, the subset labels, "lanes", four searches in flight and the overflow recovery
 *     passes work as for inner product.  Two rows whose float32 similarity scores differ may round to the same distance: inside
 *     such a tie the order is that of the similarity score;
 *   - a row with |x~|^2 beyond the split's limit (fp16: 33538048, just under 2^25; bf16: 2^121) cannot carry its bias: the bias
 *     saturates at the limit - the row ranks behind every row within the limit unless q.x~ alone reaches the limit (|q~| |x~| >=
 *     1.6e7 for fp16) - and stat "l2_saturated_rows" counts it: a store that reports 0 has no such row;
 *   - REFUSED, each with its own vodhip_last_error: VODHIP_L2 | VODHIP_EXACT_F32, vodhip_index_score_ids / _search_ids on an L2
 *     index, vodhip_node_index_create with the flag. */
#define VODHIP_L2 0x200
/* where a caller buffer lives */
enum { VODHIP_HOST = 0, VODHIP_DEVICE = 1 };

typedef struct vodhip_index vodhip_index_t;

const char* vodhip_last_error(void);
int vodhip_version(void);

/* ---------------------------------------------------------------------------------------------
 * H1  corpus vector store.
 * Replaces: faiss.index_factory(D, "Flat", METRIC_INNER_PRODUCT | METRIC_L2 with VODHIP_L2) + index.add(float32 batch)
 *           (src/vod_search/faiss_search/build.py:51-81) and the faiss.write_index/read_index
 *           round trip (src/vod_search/factory.py:167, src/vod_search/faiss_search/server.py:42).
 * The store is a row-major [capacity, dim_padded] fp16/bf16 matrix in HBM on `device`
 * (dim padded with zeros to a multiple of 64).  Rows get ids 0,1,2,... in insertion order.
 * ------------------------------------------------------------------------------------------- */
int vodhip_index_create(int device, int64_t dim, int store_dtype /* VODHIP_F16 | VODHIP_BF16, optionally | VODHIP_EXACT_F32 or | VODHIP_L2 */,
                        int64_t capacity_rows, vodhip_index_t** out);
int vodhip_index_destroy(vodhip_index_t* index);

/* Append `n_rows` row-major [n_rows, dim] vectors of `src_dtype` living in host or device memory.
 * Values are rounded to the store dtype (round-to-nearest-even).  Synchronous for host sources
 * (the call returns when the rows are resident); async on `stream` for device sources.
 * Host sources are pipelined in 64 MB slices: a pinned / registered source is read in place by the DMA engine; a pageable one
 * (NumPy array, .npy memory map) is copied into two pinned staging slots by CPU threads (param "ingest_threads", 0 = auto)
 * while the previous slice is in flight.  Pass the WHOLE array in one call: slicing it on the caller's side serialises the stages. */
int vodhip_index_add(vodhip_index_t* index, const void* rows, int64_t n_rows, int src_dtype,
                     int src_location, void* stream);
int vodhip_index_reset(vodhip_index_t* index);               /* ntotal := 0 (capacity kept) */
int vodhip_index_ntotal(const vodhip_index_t* index, int64_t* out);
int vodhip_index_dim(const vodhip_index_t* index, int64_t* out);
int vodhip_index_capacity(const vodhip_index_t* index, int64_t* out);
/* raw view of the store (device pointer, row stride in elements) for persistence / tests; the stride of a VODHIP_L2 store
 * includes its three bias columns (columns [dim, dim + 3) of every row), then the zero padding */
int vodhip_index_data(const vodhip_index_t* index, void** dev_ptr, int64_t* row_stride_elems, int* store_dtype);
/* copy rows [row_begin, row_begin + n_rows) of the store, as stored (fp16/bf16, unpadded [n_rows, dim]),
 * to `dst` in host or device memory; async on `stream` for device destinations. */
int vodhip_index_get_rows(const vodhip_index_t* index, int64_t row_begin, int64_t n_rows, void* dst,
                          int dst_location, void* stream);
/* VODHIP_EXACT_F32 stores only: the float32 plane (what faiss.write_index would persist, factory.py:167) - raw view, and rows
 * [row_begin, row_begin + n_rows) unpadded [n_rows, dim] float32 into host or device memory.  -1 for a store without the plane. */
int vodhip_index_data_f32(const vodhip_index_t* index, void** dev_ptr, int64_t* row_stride_elems);
int vodhip_index_get_rows_f32(const vodhip_index_t* index, int64_t row_begin, int64_t n_rows, void* dst, int dst_location, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H2  exact brute-force inner-product top-k over the store.
 * Replaces: faiss_index.search(query_vec, k)
 *           (src/vod_search/faiss_search/server.py:72 and :84).
 * `queries` is a DEVICE pointer to row-major [nq, dim] values of `q_dtype`; they are rounded to the
 * store dtype.  Scores are fp32-accumulated dot products of the stored (rounded) values.
 * `id_base` is added to every valid id (row offset of this shard inside a sharded corpus,
 * the reference's `indices += offset` at src/vod_search/sharded_search.py:103,155 -- pads stay -1).
 * out_scores / out_ids are DEVICE pointers [nq, k].  1 <= k <= VODHIP_MAX_K.
 *
 * VODHIP_EXACT_F32 stores: the fp16 / bf16 scan is only the FILTER.  Scores are float32 dot products of the UNROUNDED query and row
 * (one fixed summation order: the same bits from every path, batch and shard), the k best by (score desc, id asc) over ALL rows -
 * guaranteed, not statistical: the scan's top-k' list (k' > k, param "exact_expand") is re-scored from the float32 plane, and the
 * device checks per query that no row outside the list can reach the k-th re-scored score, using the bound
 * |s - s~| <= |q - q~| max|x| + |q~| max|x - x~| (+ summation slack) with the norms of the actual data; a query that fails the check
 * is searched again with every row inside that band as a candidate ("Exact-f32 mode").  The queries must stay valid until finish, as
 * always; q_dtype F32 is the point of the mode, F16 / BF16 queries are taken as exact values.
 *
 * vodhip_index_search        enqueue + wait + exactness check (if a query's candidate list overflowed, that query is
 *                            searched again with thresholds seeded from its incomplete result; the exhaustive
 *                            schedule is the last resort); results are final on return.
 * vodhip_index_search_async  enqueue only.  Must be followed by vodhip_index_search_finish on the
 *                            same index before the outputs are trusted.  Up to 4 searches may be in flight
 *                            (same stream; they share the workspace in stream order); finish completes the
 *                            OLDEST one and waits for it alone, so a caller that runs one search ahead never
 *                            leaves the device idle while the host checks the exactness flag.  The query and
 *                            output buffers of a search must stay valid and unmodified until its finish.
 * ------------------------------------------------------------------------------------------- */
#define VODHIP_MAX_K 2048
int vodhip_index_search(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, int k,
                        int64_t id_base, float* out_scores, int64_t* out_ids, void* stream);
int vodhip_index_search_async(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, int k,
                              int64_t id_base, float* out_scores, int64_t* out_ids, void* stream);
int vodhip_index_search_finish(vodhip_index_t* index, void* stream);

/* H2i  scores of LISTED rows, and the top-k over a list: the dense counterpart of `ids` in the reference's SearchClient.search.
 * Replaces: nothing the reference's dense engine does - its faiss client drops `ids` (src/vod_search/faiss_search/client.py:70); its
 *           Elasticsearch client honours it with a `terms` filter on the section id, so that only listed sections can be hits, and
 *           returns labels = scores > -inf (src/vod_search/es_search/client.py:145,177-183).  The gold-section lookup of the hybrid
 *           search (src/vod_dataloaders/core/search.py:42-50) is such a request.  (faiss calls the primitive compute_distance_subset.)
 * `ids_dev` is a DEVICE int64 [nq, m] array of section ids; queries as in H2 (rounded to the store dtype, saturating; VODHIP_EXACT_F32
 * stores score the unrounded query against the float32 rows - the SAME BITS vodhip_index_search returns for that pair).  A slot is
 * ABSENT, and scores -inf, when it is empty (id < 0), out of range (id - id_base outside [0, ntotal): rows past ntotal are never read)
 * or ineligible: `q_labels_dev` (DEVICE int32 [nq, n_per_query], NULL = unrestricted) lists the subset labels a query allows, with the
 * rule of vodhip_index_set_query_labels (-1 = empty slot, all -1 = unrestricted).  The labels are an ARGUMENT here, not index state.
 * Every (query, row) pair is summed in one fixed order: its bits do not depend on the slot, on m, on nq or on the launch.  A NaN score
 * is written as computed.
 *   vodhip_index_score_ids   the aligned form: out_scores DEVICE float32 [nq, m], slot for slot; any m >= 1.
 *   vodhip_index_search_ids  the k best DISTINCT listed rows by (score desc, id asc) - a listed id counts once, NaN and -inf never
 *                            enter - as out_scores / out_ids DEVICE [nq, k], pads (-inf, -1); 1 <= k <= VODHIP_MAX_K,
 *                            m <= VODHIP_MAX_LISTED (the aligned scores live in a hipMallocAsync temporary on `stream`).
 * The calls only enqueue work: the outputs are complete on `stream`; nothing synchronises with the host and there is no finish -
 * nothing here can overflow.  They use neither the index's search workspace nor its query labels: a call may run on any stream while
 * searches of the same index are in flight, and from several threads; it must not overlap add / reset / set_row_labels (the rule of
 * a search).  m < 1, m above the limit of the top-k form, k out of range, or labels without row labels return < 0. */
#define VODHIP_MAX_LISTED 8192
int vodhip_index_score_ids(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m,
                           int64_t id_base, const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                           float* out_scores, void* stream);
int vodhip_index_search_ids(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m,
                            int k, int64_t id_base, const int32_t* q_labels_dev, int n_per_query, float* out_scores,
                            int64_t* out_ids, void* stream);

/* H2w  the WEIGHTED SUM of listed rows (kernels_listed.hip): the backward of H2i's scores with respect to the query, and by itself the
 * priority-sampling estimate of the posterior mean (ids and exp(log_weight) of H2s), a truncated posterior mean, or a float32 row fetch.
 *     out[q, d] = sum over the PRESENT slots j with weights[q, j] != 0 of weights[q, j] * x~[ids[q, j] - id_base, d]
 * `ids_dev` DEVICE int64 [nq, m], `weights_dev` DEVICE float32 [nq, m], `out` DEVICE float32 [nq, dim], dense; any m >= 1.
 * PRESENCE is H2i's rule (the same device function decides it): id >= 0, id - id_base in [0, ntotal), and the row's label among the
 * query's `q_labels_dev` (an argument; NULL or all -1 = unrestricted).  An ABSENT slot contributes nothing WHATEVER its weight, NaN and
 * +-inf included (an upstream gradient at a -inf score is often NaN).  A present slot whose weight is exactly 0.0 (either sign) is
 * skipped too: its row is not read and cannot contribute NaN or inf.  A query whose slots are all skipped gets the zero row.  A
 * duplicate id contributes once per slot.  A NaN weight on a present slot makes that query's row NaN, and no other's.
 * PLANE: fp16 / bf16 stores sum the stored 16-bit rows, widened exactly to float32; VODHIP_EXACT_F32 stores sum the float32 plane -
 * the plane their H2i scores come from.  Products and sums are float32, each product fused into its add, subnormals kept.
 * ORDER: one summation order per (query, column), fixed by that query's own ids / weights row and the store's width: it does not
 * depend on nq, on the query's place in the batch or on the launch; no atomics.  (Slots in runs of 8 in increasing order, the 4 runs of
 * a 32-slot chunk as ((0 + 1) + 2) + 3, the chunks in increasing order.)
 * The call only enqueues work on `stream` and never synchronises with the host; lists longer than one chunk keep their partial sums
 * in a hipMallocAsync temporary on `stream` of at most VODHIP_SUM_IDS_TEMP_BYTES (or one query's), a slice of the batch at a time.
 * Like H2i it reads the store and the row labels only: it may run on any stream beside searches in flight and from several threads,
 * and must not overlap add / reset / set_row_labels.  REFUSED (< 0, vodhip_last_error): m < 1, labels without row labels, n_per_query
 * outside [1, 64], NULL buffers with nq > 0, and an L2 index (its rows carry bias columns and its scores are distances).  nq == 0
 * returns 0 and writes nothing. */
#define VODHIP_SUM_IDS_TEMP_BYTES (256ll << 20)
int vodhip_index_sum_ids(vodhip_index_t* index, const int64_t* ids_dev, const float* weights_dev, int64_t nq, int64_t m, int64_t id_base,
                         const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query, float* out /* DEVICE [nq, dim] */,
                         void* stream);

/* H2p. The exact softmax normaliser of the retriever over the WHOLE store (kernels_partition.hip):
 *     log Z_beta(q) = log sum_{z < ntotal, eligible} exp(beta * <q~, x~_z>) = beta * out_max[q] + out_log_rel[q]
 * with out_max[q] = the largest score (the bits vodhip_index_search returns at k = 1) and out_log_rel[q] = log sum exp(beta (s - max))
 * >= 0.  Two words, not one: beta * max can be tens of thousands, where the float32 spacing would swallow log_rel; callers who want one
 * number add them.  Replaces: nothing in the reference - it never normalises over the store; this is the denominator its truncated
 * objectives (top-k + samples) approximate, so logsumexp(beta * topk) - log Z is the posterior mass a result list covers.
 * Queries as in H2 (rounded to the store dtype, saturating).  A row counts when it is below ntotal, its score is not NaN (a search
 * leaves NaN out too) and `q_labels_dev` (DEVICE int32 [nq, n_per_query], NULL = unrestricted; the rule of
 * vodhip_index_set_query_labels; an ARGUMENT, not index state) allows it.  No eligible row (an empty index included): (-inf, -inf).
 * A +inf score: (+inf, +inf).  One scan of the store on the MFMA path with an online log-sum-exp in place of the top-k; the score
 * matrix is never materialised.  ONE summation order per query, fixed by ntotal and the padded width alone: a query's two words are
 * the same bits whatever the batch around it, and on every repeat.
 * out_max / out_log_rel: DEVICE float32 [nq], complete on `stream`; the call only enqueues work and uses neither the index's search
 * workspace nor its query labels (its temporaries are hipMallocAsync on `stream`): it may run beside searches in flight; it must not
 * overlap add / reset / set_row_labels.  nq == 0 returns 0 and writes nothing.
 * REFUSED, each with its own vodhip_last_error: NULL index / pointers with nq > 0, q_dtype outside 0..2, beta not finite or <= 0,
 * n_per_query outside 1..64, labels without row labels, a VODHIP_L2 store (its scores are not similarities), a VODHIP_EXACT_F32 store
 * (this pass scores the rounded plane). */
int vodhip_index_log_partition(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                               const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                               float* out_max /* DEVICE [nq] */, float* out_log_rel /* DEVICE [nq] */, void* stream);

/* H2t. The moments of the score under that softmax (kernels_stats.hip): with p(z | q) = exp(beta s_z - log Z_beta(q)), s_z = <q~, x~_z>,
 *     out_mean_rel[q] = E_p[s] - out_max[q] <= 0,    out_var[q] = Var_p[s] >= 0,
 *     d log Z_beta / d beta = out_max + out_mean_rel,   d^2 log Z_beta / d beta^2 = out_var,
 *     entropy H(p(. | q)) = out_log_rel - beta * out_mean_rel   (two non-negative terms: no beta * max cancellation).
 * out_max / out_log_rel are the bits vodhip_index_log_partition returns for the same query; eligibility, queries, labels, stream and
 * concurrency rules are H2p's.  ONE scan: H2p's with two more accumulators per (query, 256-row tile) - with d = s - m <= 0 (m the
 * tile's maximum) and e = exp(beta d), the very value H2p sums, a = sum e d and b = sum e d^2 in float32, same-sign sums in H2p's
 * order; a row whose e is 0 (underflow, a -inf score) adds +0.  The finish re-centres the tiles on the maximum in double,
 * A = sum_t c_t (a_t + D_t l_t), B = sum_t c_t (b_t + 2 D_t a_t + D_t^2 l_t), L' = sum_t c_t l_t with D_t = m_t - max and
 * c_t = exp(beta D_t), in increasing tile order: mean_rel = A / L', var = max(0, B / L' - (A / L')^2), each rounded to float32 once.
 * ONE order per query, fixed by ntotal and the padded width alone: the four words are the same bits whatever the batch around the
 * query, and on every repeat; there are no atomics.
 * No eligible row (or scores that are all -inf): (-inf, -inf, NaN, NaN).  A +inf score: (+inf, +inf, NaN, NaN).  Eligible rows that all
 * score the same: mean_rel == 0 and var == 0 exactly.
 * All four outputs: DEVICE float32 [nq], complete on `stream`.  Temporaries are hipMallocAsync on `stream`: the staged queries and 16
 * bytes per (query, tile); batches run in slices of 64 .. 1024 queries chosen so that the partials stay at or below
 * VODHIP_POSTERIOR_TEMP_BYTES unless a 64-query slice alone needs more.  The call only enqueues work.
 * nq == 0 returns 0 and writes nothing; a refused call writes nothing.  REFUSED as H2p, and a NULL out_mean_rel / out_var. */
int vodhip_index_posterior_stats(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                 const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                                 float* out_max, float* out_log_rel, float* out_mean_rel, float* out_var /* DEVICE [nq] each */,
                                 void* stream);

/* H2d. TWO posteriors over the same rows (kernels_divergence.hip): pair i is (queries_a[i], queries_b[i]) with beta_a and beta_b,
 *     p = softmax(beta_a s_a),  r = softmax(beta_b s_b),  s_a = <a~, x~_z>,  s_b = <b~, x~_z>  (the scan's scores, H2p)
 * over the rows eligible for the PAIR: z < ntotal, neither score NaN, allowed by the pair's labels (one label row per pair).  Eight words:
 *     out_max_a, out_log_rel_a, out_mean_rel_a = E_p[s_a] - max_a <= 0,  out_cross_rel_ab = E_p[s_b] - max_b <= 0,
 *     out_max_b, out_log_rel_b, out_mean_rel_b = E_r[s_b] - max_b <= 0,  out_cross_rel_ba = E_r[s_a] - max_a <= 0,
 *     H(p) = log_rel_a - beta_a mean_rel_a,   H(p, r) = log_rel_b - beta_b cross_rel_ab,
 *     KL(p || r) = (log_rel_b - log_rel_a) + (beta_a mean_rel_a - beta_b cross_rel_ab)   (and the mirror): no beta * max cancellation.
 * ONE scan, H2t's over 2 nq staged queries: pair p of a launch stages a at column p % 32 and b at column 32 + p % 32 of the 64-column
 * block p / 32, so that a lane holds both scores of a row in the same registers.  Two 16-byte partials per (pair, 256-row tile),
 * (m, l, a, c) per side: m, l, a as H2t forms them, c_ab = sum e_a (s_b - m_b) with m_b the tile's maximum of side b - same-sign, in
 * H2t's order, a row whose e_a is 0 adds +0.  The finish re-centres in double, in increasing tile order:
 * C_ab = sum_t c^a_t (c_ab_t + (m_b_t - max_b) l_a_t), cross_rel_ab = C_ab / L'_a, rounded to float32 once.
 * When no row scores NaN against exactly one side, (max, log_rel, mean_rel) of each side are the bits H2t returns for that side alone.
 * A pair's eight words are the same bits whatever the batch around it, at any position, and on every repeat; there are no atomics.  A
 * pair whose two queries and betas are identical has cross_rel_ab == mean_rel_a bit for bit.
 * A row with p_z > 0 that side b scores -inf: cross_rel_ab = -inf (H(p, r) = KL = +inf).  A row side a scores -inf adds nothing to
 * side a.  A side with no eligible row (or scores all -inf): (-inf, -inf, NaN); with a +inf score: (+inf, +inf, NaN); BOTH cross words
 * are NaN then and the other side's own three words are unaffected.
 * All eight outputs: DEVICE float32 [nq], complete on `stream`.  nq <= 2^19.  Temporaries are hipMallocAsync on `stream`: the staged
 * queries and 32 bytes per (pair, tile); batches run in slices of 64 .. 1024 pairs chosen as H2t's.  The call only enqueues work.
 * nq == 0 returns 0 and writes nothing; a refused call writes nothing.  REFUSED as H2t (each beta finite and > 0), and any NULL
 * query / output pointer. */
int vodhip_index_posterior_divergence(vodhip_index_t* index, const void* queries_a, const void* queries_b /* DEVICE [nq, dim] */, int q_dtype,
                                      int64_t nq, float beta_a, float beta_b,
                                      const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                                      float* out_max_a, float* out_log_rel_a, float* out_mean_rel_a, float* out_cross_rel_ab,
                                      float* out_max_b, float* out_log_rel_b, float* out_mean_rel_b, float* out_cross_rel_ba /* DEVICE [nq] each */,
                                      void* stream);

/* H2m. The posterior mean of the stored rows under that softmax (kernels_posterior.hip) = the gradient of log Z with respect to q:
 *     out_mean[q, :] = sum_{z < ntotal, eligible} p(z | q) x~_z,   p(z | q) = exp(beta <q~, x~_z> - log Z_beta(q)),
 *     d log Z_beta / d q = beta * out_mean[q, :].
 * out_max / out_log_rel are the bits vodhip_index_log_partition returns for the same query (its three launches run first, unchanged);
 * eligibility, queries, labels, stream and concurrency rules are H2p's.  A second scan turns each 256-row tile's scores into weights
 * exp(beta (s - m_ref)), rounded ONCE to the store dtype, and contracts them with the tile's rows on the MFMA (float32 accumulate);
 * m_ref is the largest score of the tile's group of VODHIP_POSTERIOR_GROUP_ROWS consecutive rows, so a group's largest weight is
 * exactly 1.  fp16 stores: weights are kept as normal fp16 numbers down to 2^-29 of the group's largest; smaller ones may be flushed
 * to zero (an absolute error below rows-per-group * 2^-29 * max |x| of the column, before the group's own weight <= 1).  The groups are
 * folded in increasing order with the weights exp(beta (m_g - max) - log_rel).  ONE order per (query, column), fixed by ntotal and the
 * padded width alone: a mean row is the same bits whatever the batch around it and on every repeat; there are no atomics.
 * No eligible row, or a +inf score: the two words as in H2p, the mean row all zeros.
 * NON-FINITE STORED VALUES: an excluded row has weight 0, and 0 * NaN is NaN on the MFMA.  A column in which any row of a scanned
 * 256-row tile holds a NaN or an infinity - an excluded row, a row past ntotal inside the last tile or a stale row behind a reset
 * included - is NaN in every query's mean; the other columns and the two scalar words are unaffected.  There is no sanitising pass.
 * out_mean: DEVICE float32 [nq, dim].  Temporaries are hipMallocAsync on `stream`: the staged queries and partials of H2p, and the
 * group accumulators, groups * slice * dim_pad * 4 bytes; batches run in slices of 64 .. 1024 queries chosen so that the accumulators
 * stay at or below VODHIP_POSTERIOR_TEMP_BYTES (256 MiB) unless a 64-query slice alone needs more.
 * nq == 0 returns 0 and writes nothing; a refused call writes nothing.  REFUSED as H2p (same messages), and a NULL out_mean.
 * VODHIP_POSTERIOR_TEMP_BYTES is the DEFAULT budget of every sliced scan (posterior_stats, posterior_divergence, rank_ids / count_above /
 * scan_score_ids, range_search, posterior_mean, posterior_expectation and its backward, sample_posterior).  The index parameter
 * "scan_temp_bytes" (vodhip_index_set_param; 0 = this default, >= 1 = that many bytes, negative refused) replaces it per index: a
 * testing and memory-tuning knob.  It changes the slice - clamp(budget / per-query bytes / 128 * 128, 64, 1024) queries, or pairs for
 * posterior_divergence - and nothing else: results are the same bits under any budget.  The stats "last_scan_slice" and
 * "last_scan_per_query_bytes" report what the last sliced call of the index used; "scan_temp_bytes" reads the budget back. */
#define VODHIP_POSTERIOR_GROUP_ROWS 16384
#define VODHIP_POSTERIOR_TEMP_BYTES (256ll << 20)
int vodhip_index_posterior_mean(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                                float* out_max /* DEVICE [nq] */, float* out_log_rel /* DEVICE [nq] */,
                                float* out_mean /* DEVICE [nq][dim] */, void* stream);

/* H2e. The posterior EXPECTATION of a per-row value table under that softmax (kernels_readout.hip): exact attention with the store as
 * keys and the table as values - the mass per class (a one-hot table), a soft k-NN read-out, a posterior mean in another space:
 *     out_values[q, c] = sum_{z < ntotal, eligible} p(z | q) v~[z, c],   p(z | q) = exp(beta <q~, x~_z> - log Z_beta(q)).
 * THE TABLE.  vodhip_index_set_row_values: `values` [n_rows][n_cols] of src_dtype (0 = f16, 1 = bf16, 2 = f32), HOST or DEVICE
 * (`location`); n_rows must equal ntotal, 1 <= n_cols <= 256 (wider tables are refused); values == NULL clears the table.  The index
 * keeps a copy on its device in the STORE dtype, rounded as the rows are (saturating), laid out [tiles * 256][c_pad] with c_pad =
 * 64 * ceil(n_cols / 64); pad columns and the rows from n_rows to the end of the last 256-row tile are written as zero.  The call waits
 * for `stream`; like set_row_labels it refuses while searches are in flight and must not overlap a read-out.  vodhip_index_reset drops
 * the table.  Rows added after the table was set leave it short: the read-out is then refused with a message that names both row
 * counts.  Saving and reloading an index (HipFlatIndex.save / HipFlatIndex.load write and read the rows) does NOT carry the table:
 * set it again after a load.
 * vodhip_index_row_values_info: the table's (n_rows, n_cols), (0, 0) when there is none; either pointer may be NULL.
 * THE CALL.  out_max / out_log_rel are the bits vodhip_index_log_partition returns for the same query; eligibility, queries, labels,
 * stream and concurrency rules are H2p's.  ONE scan of the store (H2m runs two): per group of VODHIP_READOUT_GROUP_ROWS consecutive
 * rows and per 256-row tile in increasing order, H2p's epilogue gives the tile maximum m_t, the exponentials e = expf(beta (s - m_t))
 * and their sum (the partial that H2p's finish folds); a running maximum M per query either rescales the group's accumulator by
 * expf(beta (M - m_t)) (m_t > M, then M = m_t) or shrinks the tile's weights by gamma = expf(beta (m_t - M)); the weights e * gamma are
 * rounded ONCE to the store dtype - one expf per (row, query) - and contracted with the tile's table rows on the MFMA (float32
 * accumulate).  fp16 stores keep a weight as a normal fp16 number down to 2^-29 of the running maximum's weight; smaller ones may be
 * flushed to zero (an absolute error below rows-per-group * 2^-29 * max |v| of the column).  The groups are folded in increasing order
 * with the weights expf(beta (M_g - max) - log_rel).
 * ONE order per (query, column), fixed by ntotal, the padded width of the store and c_pad alone: a row of the result is the same bits
 * whatever the batch around it and on every repeat; there are no atomics.
 * No eligible row, or a +inf score: the two words as in H2p, the value row all zeros.
 * NON-FINITE TABLE VALUES (H2m's contract): an excluded row has weight 0, and 0 * NaN is NaN on the MFMA.  A NaN or an infinity in
 * column c of the table - in an excluded row included - makes column c of every query NaN; the other columns and the two scalar words
 * are unaffected.  There is no sanitising pass.
 * out_values: DEVICE float32 [nq, n_cols].  Temporaries are hipMallocAsync on `stream`: the staged queries and partials of H2p, and the
 * group accumulators, groups * slice * c_pad * 4 bytes; batches run in slices of 64 .. 1024 queries chosen so that partials and
 * accumulators stay at or below VODHIP_POSTERIOR_TEMP_BYTES unless a 64-query slice alone needs more.  The call only enqueues work.
 * nq == 0 returns 0 and writes nothing; a refused call writes nothing.  REFUSED as H2p (L2 and VODHIP_EXACT_F32 stores, bad arguments,
 * labels without row labels), and: no table, a table whose n_rows is not ntotal, a NULL out_values. */
#define VODHIP_READOUT_GROUP_ROWS 4096
#define VODHIP_READOUT_MAX_COLS 256
int vodhip_index_set_row_values(vodhip_index_t* index, const void* values, int64_t n_rows, int64_t n_cols, int src_dtype, int location,
                                void* stream);
int vodhip_index_row_values_info(const vodhip_index_t* index, int64_t* n_rows, int64_t* n_cols);
int vodhip_index_posterior_expectation(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                       const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                                       float* out_max /* DEVICE [nq] */, float* out_log_rel /* DEVICE [nq] */,
                                       float* out_values /* DEVICE [nq][n_cols] */, void* stream);

/* H2b. The gradient of H2e's read-out in the QUERY (kernels_readout_grad.hip): with y = out_values of H2e, g = grad_values = dL / dy,
 *     out_grad_queries[q, :] = beta * sum_{z < ntotal, eligible} p(z | q) (u_z - ubar_q) x~_z,
 *     u_z = sum_c g[q, c] v~[z, c],   ubar_q = sum_c g[q, c] y[q, c]:
 * a posterior mean with signed, centred per-(row, query) weights (the centring is inside the weight: a table column of ones cancels
 * exactly, not catastrophically).  INPUTS: the queries, beta and labels of the forward call and its three outputs - max_score, log_rel
 * (DEVICE [nq]) and values (DEVICE float32 [nq][n_cols]) - so no partition scan runs in front: ONE scan of the store.  Eligibility,
 * queries, labels, stream and concurrency rules are H2p's; the table is the one H2e reads.
 * g is staged per query: k_q = the exponent of max_c |g[q, c]|, g^ = g * 2^-k_q (exact; the largest entry in [1, 2), so a loss gradient
 * of 1e-6 does not flush in fp16) rounded ONCE to the store dtype; ubar_q = float32 of sum_c g^ y summed in double in increasing c over
 * the columns with g^ != 0; R_q = the power of two above (sum_c |g^[q, c]| vmax_c + |ubar_q|) (1 + 2^-10), vmax_c the largest finite
 * |v~[., c]|, so that no weight exceeds 1.  vmax is computed by the first call after the table was set (one reduction; that call waits
 * for `stream` once) and kept beside the table; setting, clearing or resetting the table drops it.
 * The scan has H2e's geometry - groups of VODHIP_READOUT_GROUP_ROWS rows, 64 queries, the running maximum with rescaling - split over
 * chunks of 192 store columns; per 256-row tile the scores and u come from the shared K loop (u with the table as rows and g^ as
 * queries), the weights round16(e * gamma * ((u - ubar_q) / R_q)) are contracted with the tile's rows on the MFMA (float32 accumulate);
 * the groups are folded in increasing order with expf(beta (M_g - max_score) - log_rel), M_g the group's own maximum, and the row is
 * multiplied by beta and by 2^k_q R_q.  fp16 stores keep a weight as a normal fp16 number down to 2^-29 of the running maximum's.
 * ONE order per (query, column), fixed by ntotal, the padded width of the store and c_pad alone: a row of the result is the same bits
 * whatever the batch around it and on every repeat; there are no atomics.  Scaling g[q, :] by a power of two scales the row by exactly
 * that power (unless it leaves float32's range).
 * ZERO ROWS, exact bits: a query without a finite max_score (no eligible row, a +inf score), an all-zero g[q, :].
 * NON-FINITE INPUT.  A NaN or an infinity in g[q, :] makes row q all NaN and leaves the other rows untouched; so does one in a y[q, c]
 * whose g^[q, c] is not zero - H2e returns such a column for a non-finite table entry.  A NaN or an infinity in the table in a row that
 * is ELIGIBLE for query q makes u of that row, and row q, NaN; in a row that is not eligible it does nothing through u (the weight is
 * selected as +0 after the product).  A stored NaN or infinity in column d of any scanned tile makes column d of every scanned query
 * NaN (H2m's contract: 0 * NaN on the MFMA).  There is no sanitising pass.
 * out_grad_queries: DEVICE float32 [nq][dim].  Temporaries are hipMallocAsync on `stream`: the staged queries and g^, the group
 * accumulators, groups * slice * dim_pad * 4 bytes, and the group maxima; batches run in slices of 64 .. 1024 queries chosen so that
 * they stay at or below VODHIP_POSTERIOR_TEMP_BYTES unless a 64-query slice alone needs more.  The call only enqueues work (but see
 * vmax).  nq == 0 returns 0 and writes nothing; a refused call writes nothing.  REFUSED as H2e, and: a NULL max_score, log_rel, values,
 * grad_values or out_grad_queries.
 * NOT BUILT: the gradient in beta, tables wider than VODHIP_READOUT_MAX_COLS, second derivatives.  The gradient in the table is H2a. */
int vodhip_index_posterior_expectation_backward(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                                const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                                                const float* max_score /* DEVICE [nq] */, const float* log_rel /* DEVICE [nq] */,
                                                const float* values /* DEVICE [nq][n_cols] */, const float* grad_values /* DEVICE [nq][n_cols] */,
                                                float* out_grad_queries /* DEVICE [nq][dim] */, void* stream);

/* H2a. The ADJOINT of H2e's read-out, its gradient in the value table (kernels_readout_adjoint.hip): with W = weights,
 *     out[z, c] = sum_{q < nq, z eligible for q} p(z | q) W[q, c]     (P^T W: DEVICE float32 [ntotal][n_cols]),
 * a reduction over the QUERIES per stored row.  W = dL / dy gives dL / dv of H2e's y = P v; one column of ones the exact posterior mass
 * every stored row receives from the batch.  The call reads no value table: n_cols (1 .. VODHIP_READOUT_MAX_COLS) is the weights' own
 * width.  INPUTS: the queries, beta and labels of a forward call (H2p, H2m, H2e, ..) and its two words max_score, log_rel (DEVICE [nq]),
 * so no partition scan runs in front: ONE scan of the store.  Eligibility, queries, labels, stream and concurrency rules are H2p's.
 * W is staged per COLUMN: k_c = the exponent of max_q |W[q, c]| over the whole batch (0 for a column of zeros), W^ = W * 2^-k_c (exact;
 * the largest entry in [1, 2), so a loss gradient of 1e-6 does not flush in fp16) rounded ONCE to the store dtype; the output column is
 * multiplied by 2^k_c, which is exact (unless it leaves float32's range).  Scaling a column of W by a power of two scales that output
 * column by exactly that power.
 * One workgroup owns 64 consecutive stored rows and walks the batch in tiles of 256 queries, in query order: the scores come from the
 * shared K loop with its operands exchanged (the same bits as every other scan), the weights round16(expf(min(0, beta (s - max_score)) -
 * log_rel)) are contracted with the tile's W^ rows on the MFMA (float32 accumulate); fp16 stores scale the weight by 2^15 before the
 * rounding, so it stays a normal fp16 number down to 2^-29.  Batches above 1024 queries run in slices of 1024: the first slice stores,
 * later slices add to `out` in slice order.  ONE order per (row, column), fixed by the queries' positions in the batch alone: an element
 * does not depend on ntotal, on the other rows or on the grid, and is the same bits on every repeat; there are no atomics, no partials
 * and no fold.  accumulate != 0: the first slice adds to what `out` holds as well (accumulate on a zeroed buffer gives the plain call's
 * bits).
 * WEIGH +0, exact: a query without finite (max_score, log_rel) (no eligible row, a +inf score), a row >= ntotal, a NaN score (a stored
 * row or a query with a NaN component), a row the query's labels do not allow.  Queries whose W row is zero change no bit of `out`.
 * NON-FINITE INPUT.  A NaN or an infinity in column c of W makes column c of every output row NaN; the other columns are unaffected.
 * Temporaries are hipMallocAsync on `stream`: the staged queries and weights of a slice and the column exponents.  The call only
 * enqueues work.  nq == 0 zero-fills `out` unless accumulating; ntotal == 0 is a no-op; a refused call writes nothing.  REFUSED as H2p,
 * and: n_cols outside [1, 256], a NULL weights (nq > 0) or out.
 * NOT BUILT: L2 and exact_f32 stores, weights wider than VODHIP_READOUT_MAX_COLS.  The gradient in the STORED ROWS is H2k: adjoint
 * calls with W[q, :] = a_q q~_q, ceil(dim / 256) of them, give its log Z term only - the read-out term's weight p(z | q) (u_qz - ubar_q)
 * depends on the row and is not of the form P^T W. */
int vodhip_index_posterior_adjoint(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                   const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                                   const float* max_score /* DEVICE [nq] */, const float* log_rel /* DEVICE [nq] */,
                                   const float* weights /* DEVICE [nq][n_cols] */, int64_t n_cols /* 1 .. 256 */, int accumulate,
                                   float* out /* DEVICE [ntotal][n_cols] */, void* stream);

/* H2k. The posterior's gradient in the STORED ROWS (kernels_key_grad.hip): with a = grad_log_z, G = grad_values, y = values,
 *     out[z, d] = beta * sum_{q < nq, z eligible for q} p(z | q) c_qz q~[q, d]     (DEVICE float32 [ntotal][dim]),
 *     c_qz = a_q + (u_qz - ubar_q),   u_qz = sum_c G[q, c] v~[z, c],   ubar_q = sum_c G[q, c] y[q, c]:
 * up to rounding the gradient of sum_q a_q log Z_q + sum_qc G_qc y_qc (H2p's log Z, H2e's y = P v~ on the attached table) in the stored
 * values x~ as stored - the rounding of the rows at ingest is passed straight through.  With H2b (queries) and H2a (table) the exact
 * attention over the store is differentiable in all three operands.  grad_log_z (DEVICE [nq]) or NULL = zero; grad_values (DEVICE
 * float32 [nq][n_cols]) or NULL = zero, given together with `values`, the forward's out_values; at least one of the two.  With
 * grad_values NULL no table is read and none needs to be attached.  INPUTS besides: the queries, beta and labels of the forward call and
 * its two words max_score, log_rel (DEVICE [nq]), so no partition scan runs in front.  Eligibility, queries, labels, stream and
 * concurrency rules are H2p's; vmax is H2b's cached one (the first call that needs it waits for `stream` once).
 * SCALES, batch-wide.  k = the exponent of the largest finite |G| of the batch (of the largest |a| without G or with G all zero);
 * G^ = round16(G 2^-k), a' = a 2^-k in float32, ubar_q as H2b forms it from G^; B_q = |a'_q| + sum_c |G^_qc| vmax_c + |ubar_q|;
 * R = the power of two above max_q B_q (1 + 2^-10).  The scales cannot be per query: the contraction runs over the queries inside the
 * MFMA, and a per-query factor could not be undone behind it.  CONSEQUENCE: on an fp16 store a query whose gradient is far below the
 * batch's largest loses relative precision (its weights sit low in fp16's range; scaled by 2^15 they stay normal down to 2^-29 R), not
 * absolute precision.  Scaling a and G together by a power of two scales `out` by exactly that power (within float32's range).
 * One workgroup owns 64 consecutive stored rows and one chunk of the store's padded columns - 256 columns without grad_values, 192
 * with (the u accumulator is live beside the scores) - and walks the batch in tiles of 256 queries, in query order: the scores from the
 * shared K loop with its operands exchanged (the same bits as every scan), u from the same loop on (G^ tile, the 64 table rows), the
 * weight round16(e * ((a'_q + (u - ubar_q)) / R)), e = expf(min(0, beta (s - max_score)) - log_rel), centred BEFORE its one rounding
 * (fp16: scaled by 2^15 first), contracted with the tile's staged queries on the MFMA (float32 accumulate); the row is multiplied by
 * beta and 2^k R.  Batches above 1024 queries run in slices of 1024: the first slice stores, later slices add in slice order.  ONE
 * order per (row, column), fixed by the queries' positions in the batch alone; no atomics in the scan, no partials, no fold: an element
 * depends on its row, the queries, their words and the batch-wide (k, R) alone and is the same bits on every repeat.  accumulate != 0:
 * the first slice adds to what `out` holds as well.
 * WEIGH +0, exact: a query without finite (max_score, log_rel), a query with B_q = 0 (a zero a_q and G[q, :]), a row >= ntotal, a NaN
 * score, a row the query's labels do not allow.  Such queries behind a batch change no bit of `out`.
 * NON-FINITE INPUT.  A NaN or an infinity in a_q, in G[q, :] or in a y[q, c] whose G^[q, c] is not zero (or scales beyond float32)
 * makes EVERY element of `out` NaN: the query weighs on every row, as it would in a dense softmax.  A non-finite table entry in a row
 * eligible for a query with G^ != 0 makes that row's u, and the row of `out`, NaN.  There is no sanitising pass.
 * Temporaries are hipMallocAsync on `stream`.  The call only enqueues work (but see vmax).  nq == 0 zero-fills `out` unless
 * accumulating; ntotal == 0 is a no-op; a refused call writes nothing.  REFUSED as H2p (an L2 index and a VODHIP_EXACT_F32 store with
 * their own messages), and: grad_log_z and grad_values both NULL, grad_values without values, grad_values without an attached table or
 * with one of another row count, a NULL out.
 * NOT BUILT: the form in which each wave owns a column range and the scores are computed once per tile (K-loop steps K + K per tile
 * against this design's chunks * (K + slices), K = dim_pad / 64; it needs a weight exchange through the LDS and half-tiles to fit
 * 160 KB); the gradient of the listed scores (H2i) in the rows, a sparse index_add; L2 and exact_f32 stores; an HTTP route; the
 * process-group engine; the gradient in beta. */
int vodhip_index_posterior_key_gradient(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                        const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                                        const float* max_score /* DEVICE [nq] */, const float* log_rel /* DEVICE [nq] */,
                                        const float* grad_log_z /* DEVICE [nq], or NULL */, const float* values /* DEVICE [nq][n_cols], or NULL */,
                                        const float* grad_values /* DEVICE [nq][n_cols], or NULL */, int accumulate,
                                        float* out /* DEVICE [ntotal][dim] */, void* stream);

/* H2u. Stored rows CHANGED IN PLACE (kernels_update.hip): where H2k's gradient goes, and a partial refresh of the store by id.
 *     VODHIP_UPDATE_SET   x[row] = rows[j]
 *     VODHIP_UPDATE_ADD   x[row] = x[row] + alpha * rows[j]     (float32: p = alpha * rows[j] rounded, then the sum rounded - no fma)
 * LISTED form (ids != NULL): slot j targets row ids[j] - id_base.  DENSE form (ids == NULL): slot j targets row row_begin + j; id_base
 * is not read.  `rows` is [n, dim] of src_dtype (F16 / BF16 / F32), at `location` as `ids` is.
 * EVERY plane the store keeps is written in the same launch, with the bytes vodhip_index_add writes for the same final values: the
 * 16-bit plane (rounded, saturating, pad columns zero), an L2 store's three bias columns (from the values as stored, in the ingest's
 * order of summation), a VODHIP_EXACT_F32 store's float32 plane and its two per-row statistics.  After the call the store equals, byte
 * for byte, one freshly built by vodhip_index_add from the final rows.  ADD's `old` is the float32 row of a VODHIP_EXACT_F32 store -
 * the master copy - and the 16-bit row widened anywhere else: there the 16-bit row IS the master copy, and a step below half a unit of
 * its last place is lost.  ntotal, the row labels and the value table (H2e) are NOT touched: a table attached before stays attached.
 * SLOTS.  A slot whose id is negative, below id_base or not below id_base + ntotal is SKIPPED and counted (H2i's pad rule).  The same
 * id in several slots: the LAST slot is applied, SET and ADD alike (NumPy's x[ids] = rows), the others write nothing and are counted
 * as duplicates - for ADD unique ids are the contract, the count is how a caller learns it was broken.  Resolved without a sort and
 * without a race by one int32 word per capacity row (allocated by the first listed call, all zero between calls); the result is the
 * same bytes on every repeat.
 * STATS (vodhip_index_get_stat; they wait for the device): "last_update_written", "last_update_skipped", "last_update_duplicates" of
 * the last call.  "l2_saturated_rows" grows by every saturated bias an update writes: it counts saturation EVENTS since create /
 * reset, not rows now saturated - a row updated out of saturation stays counted.
 * VODHIP_EXACT_F32: the two maxima of the error bound are re-derived from the per-row statistics of the rows NOW stored before the
 * next search (8 bytes per row); a maximum left behind by a row that was replaced never made a result wrong, but it placed the
 * outlier cuts.
 * DEVICE sources only enqueue work on `stream`; HOST sources go through the ingest's staging slots and return when the rows are
 * written, as vodhip_index_add.  n == 0 is a no-op that succeeds; SET ignores alpha.  REFUSED (-1, nothing written): searches in
 * flight (the rule of vodhip_index_add), a dense range outside [0, ntotal), n < 0 or n >= 2^31 - 1, NULL rows with n > 0, a bad
 * src_dtype, location or mode, a non-finite alpha with ADD.
 * NOT BUILT: an HTTP route, the value table or the labels by id, stochastic rounding.  (Removing rows: H2r.) */
#define VODHIP_UPDATE_SET 0
#define VODHIP_UPDATE_ADD 1
int vodhip_index_update_rows(vodhip_index_t* index, const int64_t* ids /* [n], or NULL: rows row_begin .. row_begin + n */, int64_t row_begin,
                             const void* rows /* [n, dim] */, int64_t n, int src_dtype, int location /* of ids AND rows */,
                             int mode, float alpha, int64_t id_base, void* stream);

/* H2r. Stored rows REMOVED, the gaps closed in place (kernels_remove.hip, remove_fold.h): faiss IndexFlat::remove_ids.
 * LISTED form (ids != NULL): slot j removes row ids[j] - id_base.  RANGE form (ids == NULL): rows [row_begin, row_begin + n); id_base
 * is not read.  `ids` is at `location`.  The compaction is STABLE: survivors keep their order and move down, a survivor's new id is
 * its old id minus the number of removed rows below it; ntotal shrinks, the capacity stays.
 * THE CONTRACT IS THE BYTES OF vodhip_index_add: afterwards every plane the store keeps - the padded 16-bit plane with an L2 store's
 * bias columns, a VODHIP_EXACT_F32 store's float32 plane and its two per-row statistics, the row labels if set, the value table (H2e)
 * if attached - equals over rows [0, ntotal), byte for byte, an index freshly built by vodhip_index_add from the surviving rows in
 * order.  Nothing is recomputed: rows are moved whole.  The labels and the value table STAY ATTACHED, compacted the same way; the
 * table keeps value_rows == ntotal and its zero pad rows up to round_up(ntotal, 256).  Behind the last row the 16-bit plane is zero
 * and the labels are -1 for round_up(ntotal, 256) + 512 rows (what a scan's last tile can read); further stale rows up to the old
 * ntotal stay as they were, as after vodhip_index_reset + add of fewer rows: no result depends on them.
 * VODHIP_EXACT_F32: the two maxima of the error bound and the outliers are re-derived from the rows NOW stored before the next search
 * (as after H2u).  "l2_saturated_rows" counts events and is not touched.
 * SLOTS as H2u: a slot whose id is negative, below id_base or not below id_base + ntotal is SKIPPED and counted; a repeated id removes
 * its row once, the extra slots are counted as duplicates.  STATS: "last_remove_removed", "last_remove_skipped",
 * "last_remove_duplicates" (host values of the last call; no wait).
 * new_ids, when not NULL: DEVICE int64 [ntotal before the call], the new id of every old row (0-based rows of this index, as the rows
 * of the range form), -1 for a removed one; written on `stream` unless n == 0 (then nothing at all is written: the map is the identity).
 * *n_removed (may be NULL) receives the number of rows removed.  The call must learn the new ntotal: it WAITS FOR THE DEVICE ONCE
 * (`stream`), between counting and moving; the moves themselves are only enqueued.  A HOST id list is copied before that wait.
 * n == 0, or a list of which every slot is skipped, is a successful no-op that writes nothing.  Removing every row leaves ntotal == 0
 * with the table and the labels attached and empty.
 * HOW (DESIGN.md 4 "Row removal"): every survivor moves DOWN, so one launch over the store would overwrite rows another workgroup has
 * not read yet.  The rows from the first removed one are cut into slabs of "remove_slab_rows" source rows (vodhip_index_set_param:
 * a power of two in [4, 2^30], 0 = the default 65536), run in ascending order; a slab whose destination ends at or below its first
 * source row is moved by one launch, any other is packed into the BOUNCE buffer and copied from there.  The bounce buffer holds
 * min(remove_slab_rows, capacity) rows of every plane the store has (2 * dim_pad bytes a row; + 4 * dim_pad + 8 of an exact store,
 * + 4 with labels, + 2 * round_up(n_cols, 64) with a table): 100 MB at the default for 768 fp16 columns, 300 MB for an exact store;
 * allocated by the first call that needs it, freed by vodhip_index_destroy.  The result does not depend on the slab size.
 * REFUSED (-1, nothing written): searches in flight (the rule of vodhip_index_add), a range outside [0, ntotal), n < 0 or
 * n >= 2^31 - 1, a bad location, and a STALE VALUE TABLE - one that rows were added behind, so that it holds fewer rows than the index
 * (the state every read-out refuses): it is neither moved nor passed off as valid; set it again or clear it first.  After any call,
 * failed ones included, the owner table of H2u is all zero.
 * A DEVICE ERROR during the call (a failed launch, copy or allocation: -1 with the HIP error's text) is no refusal: some slabs may have
 * moved while ntotal is unchanged, so the store's contents are UNDEFINED and the caller must vodhip_index_reset (the node form:
 * vodhip_node_index_reset - earlier shards may already be compacted) and add the rows again.
 * NOT BUILT: an HTTP route, removal while a batcher serves, an unstable swap-with-tail mode, shrinking the capacity. */
int vodhip_index_remove_rows(vodhip_index_t* index, const int64_t* ids /* [n], or NULL: rows row_begin .. row_begin + n */, int64_t row_begin,
                             int64_t n, int location /* of ids */, int64_t id_base, int64_t* new_ids /* DEVICE [ntotal], or NULL */,
                             int64_t* n_removed /* HOST, or NULL */, void* stream);
/* TEST-ONLY: not part of the drop-in interface, no stability promise; the pointers are the store's own - read them, never write them.
 * Raw views of the planes beside the rows, for the byte-for-byte tests of H2u / H2r: the device pointer (NULL when the store keeps no such plane), the rows
 * that hold data and the row stride in elements.  LABELS int32 [ntotal]; VALUES the table, 16-bit [round_up(value_rows, 256)][c_pad];
 * ROW_N2 / ROW_D2 float32 [ntotal] (VODHIP_EXACT_F32); OWNER the int32 word per capacity row of H2u / H2r (zero between calls). */
#define VODHIP_PLANE_LABELS 0
#define VODHIP_PLANE_VALUES 1
#define VODHIP_PLANE_ROW_N2 2
#define VODHIP_PLANE_ROW_D2 3
#define VODHIP_PLANE_OWNER 4
int vodhip_index_plane(const vodhip_index_t* index, int which, void** dev_ptr, int64_t* n_rows, int64_t* row_stride_elems);

/* H2s. k rows drawn WITHOUT replacement from that softmax over the whole store, with priority-sampling weights
 * (kernels_sample_posterior.hip).  Gumbel-top-k: the k eligible rows with the largest keys
 *     key(q, z) = fl(fl(beta * s(q, z)) - logf(E)),   E = -log1pf(-v),   by (key desc, id asc),
 * s the float32 score of H2p's scan, and with key_{k+1} the (k+1)-th largest key
 *     log_p = beta (s - max_score) - log_rel,   log_tau = (key_{k+1} - beta max_score) - log_rel,
 *     log_weight = log_p - log(-expm1(-exp(log_p - log_tau)))   (double arithmetic on the float32 words; log_tau = -inf: log_p).
 * sum_S exp(log_weight) f(z) is an unbiased estimate of E_p[f].  NOISE: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and
 * counter (low word of g >> 2, g >> 34, qs, j), g = id_base + row, qs = query_offset + q: output word g & 3 at j = 0 is w_hi of row g,
 * at j = 1 its w_lo; v = float32((w_hi 2^32 + w_lo + 1/2) 2^-64), at most 1 - 2^-24.  A draw depends on (seed, qs, g) alone: not on
 * the batch, the sharding or the launch geometry.  query_offset >= 0, query_offset + nq <= 2^32, id_base >= 0.
 * out_max / out_log_rel are H2p's bits for the same query (its launches run first, unchanged); eligibility, queries, labels and
 * stream rules are H2p's; a row with a -inf score is never drawn.  Behind them: a key-max scan (one float per query and 256-row
 * tile), a threshold launch (theta = the (k+1)-th largest tile maximum: a lower bound of key_{k+1}), an emit scan that skips the
 * K loop of every tile without a key >= theta and appends the others' to per-query lists of 256 (k + 1 +
 * VODHIP_SAMPLE_SLACK_TILES) slots (at most the padded store), and a select launch.  The result is exact: there is no fallback pass.
 * A list can only overflow when more than VODHIP_SAMPLE_SLACK_TILES further tile maxima tie EXACTLY with theta; a slot past the
 * list is not written, the call fails ("candidate list overflow") and its outputs are undefined.
 * Outputs, DEVICE: out_ids int64 [nq][k] (pads -1), out_scores / out_log_p / out_log_weight float32 [nq][k] (pads -inf), out_keys
 * float32 [nq][k + 1] (unnormalised keys, descending, pads -inf).  Fewer than k eligible rows: pads; a query whose log Z is not
 * finite (no eligible row, a +inf score): all pads.  Batches run in slices of 64 .. 1024 queries so that the temporaries (12 bytes
 * per list slot, 12 per query and tile) stay at or below VODHIP_POSTERIOR_TEMP_BYTES unless a 64-query slice alone needs more.  The
 * call WAITS for `stream` before it returns (it reads its status words).  Its temporaries are one grow-only block that the index
 * keeps until it is destroyed (a stream-ordered pool hands its memory back at every such wait); the block is held for the length of
 * a call, so two calls on one index run one after the other, whatever their streams - searches and the other calls of this header
 * are not held up.  Stats "last_sample_overflow", "last_sample_selfcheck" (queries with fewer
 * candidates than hit tiles: never, the two scans compute a key with the same instructions), "last_sample_candidates" /
 * "last_sample_max_candidates", "last_sample_emit_groups" / "last_sample_emit_skipped", and with param "profile" = 1
 * "last_sample_ns_partition" / "_keymax" / "_threshold" / "_emit" / "_select".
 * nq == 0 returns 0 and writes nothing; a refused call writes nothing.  REFUSED as H2p (L2 and VODHIP_EXACT_F32 stores with messages
 * of their own), k outside [1, 255], a bad query_offset / id_base, a NULL output. */
#define VODHIP_SAMPLE_SLACK_TILES 2
int vodhip_index_sample_posterior(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, int k, float beta, uint64_t seed,
                                  int64_t query_offset, int64_t id_base, const int32_t* q_labels_dev /* NULL = unrestricted */,
                                  int n_per_query, float* out_max /* DEVICE [nq] */, float* out_log_rel /* DEVICE [nq] */,
                                  int64_t* out_ids /* DEVICE [nq][k] */, float* out_scores, float* out_log_p,
                                  float* out_log_weight /* DEVICE [nq][k] */, float* out_keys /* DEVICE [nq][k + 1] */, void* stream);

/* H2r. Exact RANKS over the whole store (kernels_rank.hip): at what position would a search return a given row, however deep - and how
 * many rows score above a threshold.  Replaces: nothing in the reference - its metrics see ranks only inside the truncated result
 * list, so MRR / hit@k / mean rank treat "rank 2049" and "rank 9 million" as the same miss.
 * ELIGIBLE rows are H2p's: below ntotal, scan score not NaN, allowed by `q_labels_dev`.  ORDER is the search's: scores compare by
 * their result key (-0.0 == +0.0), ties go to the smaller id.  For a threshold t and a tie id r
 *     C(q; t, r) = #{ eligible rows z : s(q, z) > t  or  (s(q, z) == t and id_base + z < r) }.
 *   vodhip_index_count_above     out_counts[q, j] = C(q; thresholds[q, j], tie_ids[q, j]); tie_ids_dev NULL: the strict count.  A NaN
 *                                threshold gives -1.
 *   vodhip_index_rank_ids        out_scores[q, j] = the SCAN's score of row ids[q, j] - the bits vodhip_index_search returns for the
 *                                pair (H2i's order of summation is another one) - and out_ranks[q, j] = C(q; that score, ids[q, j]):
 *                                the 0-based position at which a search over the eligible rows returns the row.  PRESENT is H2i's rule;
 *                                an absent slot gives (-1, -inf), a NaN score rank -1 with the score as computed.  Duplicate ids are
 *                                independent slots.
 *   vodhip_index_scan_score_ids  the scores alone (no scan of the store: the listed rows are gathered and multiplied on the MFMA with
 *                                the scan's K loop); out_rows (may be NULL): DEVICE int32 [nq, m], the local row of a present slot, -1
 *                                of an absent one - a present row with a -inf score and an absent slot both score -inf.
 * 1 <= m <= VODHIP_RANK_MAX_LISTED; the cost of the scan's epilogue is linear in m.  One scan of the store on the MFMA path with integer
 * compares in place of the top-k; nothing of size [nq, N].  Counts are integer sums: the same on every repeat and whatever the batch.
 * Temporaries are hipMallocAsync on `stream` (staged queries, the gathered rows, 12 bytes per slot), batches run in slices of 64 .. 1024
 * queries so that they stay at or below VODHIP_POSTERIOR_TEMP_BYTES unless a 64-query slice alone needs more.  The calls only enqueue
 * work and never synchronise with the host; they use neither the search workspace nor the index's query labels: they may run beside
 * searches in flight; they must not overlap add / reset / set_row_labels.  nq == 0 returns 0 and writes nothing.
 * REFUSED, each with its own vodhip_last_error: NULL index / pointers with nq > 0, q_dtype outside 0..2, m outside [1, 64], n_per_query
 * outside [1, 64], labels without row labels, VODHIP_L2 and VODHIP_EXACT_F32 stores (H2p's reasons). */
#define VODHIP_RANK_MAX_LISTED 64
int vodhip_index_count_above(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, const float* thresholds_dev,
                             const int64_t* tie_ids_dev /* NULL = strict */, int64_t m, int64_t id_base,
                             const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                             int64_t* out_counts /* DEVICE [nq][m] */, void* stream);
int vodhip_index_rank_ids(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m,
                          int64_t id_base, const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                          int64_t* out_ranks /* DEVICE [nq][m] */, float* out_scores /* DEVICE [nq][m] */, void* stream);
int vodhip_index_scan_score_ids(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m,
                                int64_t id_base, const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query,
                                float* out_scores /* DEVICE [nq][m] */, int32_t* out_rows /* DEVICE [nq][m], or NULL */, void* stream);

/* H2g. RANGE SEARCH over the whole store (kernels_range.hip): WHICH rows score above a per-query threshold - the rows H2r counts.
 * Replaces: faiss's range_search (lims, D, I) of the flat index this library stands in for; the reference never calls it.
 * Eligibility, order and the predicate are H2r's.  For thresholds[q] = t and tie_ids[q] = r (tie_ids_dev NULL: the strict test) the
 * result of query q is
 *     R(q) = { eligible rows z : s(q, z) > t  or  (s(q, z) == t and id_base + z < r) },
 * exactly the set vodhip_index_count_above counts with m = 1.  A NaN threshold gives an empty list; r past every row makes the test
 * inclusive.  The result is CSR: lims_dev int64 [nq + 1] (lims[0] = 0), and at positions lims[q] .. lims[q + 1] of out_scores_dev /
 * out_ids_dev the scan's scores (the bits vodhip_index_search returns) and the ids id_base + z, ids ASCENDING within a query.  It is
 * a function of the store and the query alone: the same bytes in any batch, any slice and on every repeat (positions come from
 * prefix sums of integer counts, not from atomics).
 *   out_scores_dev == NULL (and out_ids_dev == NULL): the SIZING call - one scan, lims alone; it only enqueues work and never
 *     synchronises with the host.
 *   with outputs of `capacity` elements each: a second scan emits the rows; a workgroup whose tile holds no hit of its queries leaves
 *     before its K loop.  When lims[nq] > capacity the call writes the complete lims, writes only the positions below `capacity`, sets
 *     the stat "last_range_overflow" (positions not written) and returns an error whose message names both numbers.  To report that, this
 *     form reads lims[nq] and its status words back and so waits for `stream`.  Stats of the last such call: "last_range_selfcheck"
 *     ((query, tile) pairs whose emitted count differed from the counted one; never above 0), "last_range_emit_skipped" /
 *     "last_range_emit_groups" (emit workgroups that left early / in all).
 * Temporaries are hipMallocAsync on `stream`: the staged queries, 12 bytes per query and 4 bytes per (query, tile); batches run in
 * slices of 64 .. 1024 queries so that the table stays at or below VODHIP_POSTERIOR_TEMP_BYTES unless a 64-query slice alone needs
 * more.  The call uses neither the search workspace nor the index's query labels: it may run beside searches in flight; it must not
 * overlap add / reset / set_row_labels.  nq == 0 writes lims[0] = 0.
 * REFUSED, each with its own vodhip_last_error: NULL index / queries / thresholds with nq > 0, NULL lims, one of the two outputs
 * without the other, capacity < 0, q_dtype outside 0..2, n_per_query outside [1, 64], labels without row labels, VODHIP_L2 and
 * VODHIP_EXACT_F32 stores (H2p's reasons). */
int vodhip_index_range_search(vodhip_index_t* index, const void* queries, int q_dtype, int64_t nq, const float* thresholds_dev /* DEVICE [nq] */,
                              const int64_t* tie_ids_dev /* DEVICE [nq], NULL = strict */, int64_t id_base,
                              const int32_t* q_labels_dev /* NULL = unrestricted */, int n_per_query, int64_t* lims_dev /* DEVICE [nq + 1] */,
                              float* out_scores_dev /* DEVICE [capacity], or NULL */, int64_t* out_ids_dev /* DEVICE [capacity], or NULL */,
                              int64_t capacity, void* stream);

/* Optional subset filter.  The reference's SearchClient.search carries `subset_ids`; its Elasticsearch and
 * Qdrant engines restrict hits to sections whose subset id is listed (src/vod_search/es_search/client.py:185-191,
 * qdrant_search/client.py:124-136) while its faiss client ignores it (faiss_search/client.py:67-72).  Here every stored
 * row may carry an int32 label (`labels` [n_rows], host or device; NULL clears), and the next searches may pass, per
 * query, up to `n_per_query` allowed labels (DEVICE int32 [nq, n_per_query], caller-owned until cleared with NULL;
 * -1 = empty slot; a query whose slots are all -1 is unrestricted; any other value, e.g. -2 for an unknown id,
 * restricts the query).  A row is eligible iff its label is listed.
 * Results stay exact top-k over the eligible rows. */
int vodhip_index_set_row_labels(vodhip_index_t* index, const int32_t* labels, int64_t n_rows, int location, void* stream);
int vodhip_index_set_query_labels(vodhip_index_t* index, const int32_t* q_labels_dev, int n_per_query);

/* Tunables / introspection (tests and bench).
 * params: "cand_cap" (candidate slots per query and stage, default 16384), "dense_rows" (indexes up to this many rows are
 *   scored densely, default 2048), "sample_div" (the threshold bootstrap scores ~ntotal / sample_div sampled rows; 0 = auto, the default: 96, and 192
 *   for batches above 512 queries on stores of 4 M rows and more), "growth" (x100: a filter stage covers growth x the rows its threshold
 *   was calibrated on; 0 = auto, the default: 800, and 300 where sample_div is 192),
 *   "force_safe" (1 = exhaustive schedule: dense chunks of <= cand_cap rows), "tile" (0 = auto; 1 = 128x128, 42 / 46 = small-batch
 *   rings, 8 / 9 = persistent 256x256 two-slot kernel without / with the wave stagger, 14 = persistent 256x256 on the 8-phase K loop: the
 *   auto choice above 128 queries), "small_chunk_tiles", "profile" (1 = HIP events around
 *   every filter launch), "ingest_threads" (CPU threads staging pageable host rows, 0 = auto), "kflags" (timing knobs of
 *   diagnostic builds), "tile_order" (0 = default: the FILTER stages of a search walk the store's 256-row tiles in a low-discrepancy
 *   order, so that every stage samples the whole store whatever order the rows were added in; 1 = in row order; results are identical),
 *   "lanes" (0 = auto, 1, 2: with 2 lanes consecutive searches alternate between two workspaces, the second on a stream of the index's
 *   own that starts behind the work the caller's stream holds at enqueue - two searches of a caller that runs one search ahead overlap
 *   on the device; auto = 2 for batches of up to 256 queries, where a search's select / prepare launches and partly filled last
 *   rounds leave ~12 % of the device idle; results are unchanged.  STREAM ORDERING with 2 lanes: every second search in flight runs on
 *   the index's stream, so work the caller enqueues on ITS stream behind vodhip_index_search_async is NOT ordered behind that search:
 *   only vodhip_index_search_finish completes a search - a hipStreamSynchronize of the caller's stream does not; set "lanes" = 1 to keep
 *   every search on the caller's stream.  add / reset / set_row_labels refuse while searches are in flight),
 *   "exact_expand" (x100, VODHIP_EXACT_F32 stores: the scan lists k' = k * exact_expand / 100 + 16 rows per
 *   query; 0 = default: 110 for an fp16 store, 200 for bf16 as the upper limit, with k' following what the last searches of the same k
 *   needed ("exact_adapt" = 1, default; 0 = always the formula); speed only - results are exact for any value),
 *   "survivor_ring" (records per wave of the 8-phase filter kernel's survivor rings, in [0, 8192]; 0 = auto, sized by the planner for
 *   the search's largest stage, at most 1024 (8 x CUs x 1024 x 132 B = 277 MB of workspace per lane on 256 CUs); the rings are skipped
 *   when the device cannot hold them; a query block that does not fit takes the in-loop path; speed and workspace only - results are the same),
 *   "scan_temp_bytes" (the temporary budget of the sliced whole-store scans; 0 = VODHIP_POSTERIOR_TEMP_BYTES, the default: see there),
 *   "remove_slab_rows" (source rows per launch of vodhip_index_remove_rows and the rows of its bounce buffer: a power of two in
 *   [4, 2^30], 0 = the default 65536; speed and memory only - the result is the same bytes).
 * VODHIP_EXACT_F32 input range: finite float32 rows and queries of ANY magnitude whose squared norm is finite in float32 (|x| < 1.8e19)
 *   give the float32 brute-force result; values beyond the scan dtype's range (fp16: |v| > 65504) saturate in the scan copy only, and
 *   the up to 64 rows whose norm / rounding error exceeds the rest of the store's by 2x or more ("outliers") are scored exactly by
 *   every query instead of widening the error bound.  Rows with NaN / inf components never enter a result (NaN scores are dropped).
 * stats (of the search completed by the last vodhip_index_search_finish): "last_overflow" (a candidate list overflowed),
 *   "last_safe_reruns" (recovery passes run), "last_recovered_queries" (queries the first recovery pass re-searched),
 *   "last_chunks" (stages), "last_survivor_ring" (records per wave of its survivor rings, 0 = none), "last_ring_fallbacks" (query blocks
 *   with survivors that did not fit into those rings and took the in-loop path, first pass), "last_filter_launches", "last_filter_ns" (with "profile"), "last_recovery_launches",
 *   "last_recovery_ns" (the filter launches of the recovery passes, accounted separately); "exact" (1 for a VODHIP_EXACT_F32 store),
 *   "last_exact_kx" (k' of the last search), "last_exact_band_queries" (queries whose list did not prove complete and ran a band
 *   pass), "last_exact_band_passes"; "l2" (1 for a VODHIP_L2 store), "l2_saturated_rows" (rows ingested since create / reset whose
 *   bias saturated; reading it waits for the device), "last_l2_stage_ns" / "last_l2_finish_ns" (with "profile": HIP events around the
 *   query staging launch and the finish launch of the first pass). */
int vodhip_index_set_param(vodhip_index_t* index, const char* key, int64_t value);
/* Host-side planning only (no device and no HIP runtime call): the stage list a search of `nq` queries for the top `k` of
 * `ntotal` rows would run on a device with `n_cu` compute units (<= 0 = 256, the MI355X), with the given tunables (<= 0 =
 * library default; tile 0 = auto, else a filter-kernel id that vodhip_index_set_param("tile") accepts in this build - any other
 * id is refused; recovery_pass 0 = the normal schedule).  An index reads its device's CU count once, at create.
 * out: int64 [max_stages][6] = {kind (0 FILTER, 1 DENSE, 2 GMAX bootstrap), row_begin, row_end, sampled tiles, sample row
 * stride, sample groups}.  Returns the number of stages, or -1. */
int vodhip_debug_schedule(int64_t ntotal, int k, int64_t nq, int64_t cand_cap, int64_t dense_rows, int64_t sample_div,
                          int64_t growth_x100, int tile, int recovery_pass, int n_cu, int64_t* out, int max_stages);
int vodhip_index_get_stat(const vodhip_index_t* index, const char* key, int64_t* out);
/* Host-side arithmetic only (no HIP call): the bias split of a VODHIP_L2 store (vod_amd/csrc/l2_bias.h).  c = -|x~|^2 / 2 as a
 * float32 -> terms[3] = the store-dtype bits kept in the row's bias columns, consts[3] = the query constants (powers of two) they
 * meet: sum_i consts[i] * value(terms[i]) = c within 2^-28 (fp16) / 2^-126 (bf16), exactly for every half-integer within the limit;
 * no term and no constant is subnormal in the store dtype.  Returns 1 when the bias saturated (|c| beyond the limit, or not
 * finite), 0 otherwise, -1 for invalid arguments. */
int vodhip_debug_l2_split(float c, int dtype, uint16_t terms[3], float consts[3]);
/* Host-side planning only: the order in which a search's FILTER stages walk the 256-row tiles of a store of `ntotal` rows - position p
 * (stages are runs of consecutive positions) is tile (p * perm_mul) mod perm_mod; perm_mul <= 1 = positions are tiles (small stores). */
int vodhip_debug_tile_order(int64_t ntotal, int64_t* perm_mul, int64_t* perm_mod);
/* Diagnostic builds only (make ABLATION=1; production returns -1): phase stamps of workgroup 0 of the last launch of a
 * kernel (which: 0 = hybrid merge, 1 = priority sampling, 2 = in-batch flattening, 3 = the search's select kernel) as 64 pairs
 * (shader-clock cycles, 10 ns ticks of the constant 100 MHz counter), then the (begin, end) ticks of workgroups 0..63;
 * out holds n >= 256 values. */
int vodhip_debug_read_probe(int which, int64_t* out, int n);

/* ---------------------------------------------------------------------------------------------
 * H3  merge of per-shard top-k lists (multi-GPU exchange step, after the RCCL all-gather).
 * Replaces: the row-offset + stack of ShardedSearchClient (src/vod_search/sharded_search.py:92-106,
 *           198-203) and faiss IndexShards' host merge (src/vod_search/faiss_search/server.py:51-54).
 * scores/ids: DEVICE [n_shards, nq, k] (ids already global, pads -1).  Output [nq, k_out].
 * One launch merges up to 8192 entries per query; more (e.g. 8 shards x top-2048) are merged in levels through a
 * stream-ordered temporary (hipMallocAsync on `stream`); k <= 4096.
 * ------------------------------------------------------------------------------------------- */
int vodhip_merge_topk(const float* scores, const int64_t* ids, int n_shards, int64_t nq, int k,
                      int k_out, float* out_scores, int64_t* out_ids, void* stream);
/* Same, with explicit element strides between shards: lets ONE all-gather move a packed per-rank record
 * [scores f32 nq*k | ids i64 nq*k] and the merge read both parts in place. */
int vodhip_merge_topk_strided(const float* scores, int64_t shard_stride_scores, const int64_t* ids,
                              int64_t shard_stride_ids, int n_shards, int64_t nq, int k, int k_out,
                              float* out_scores, int64_t* out_ids, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H1 + H2 + H3 on several devices of one node, from ONE process: for consumers without torch.distributed (C, C++, cgo, JNI).
 * Replaces: faiss.index_cpu_to_all_gpus(index, co) with co.shard = True, i.e. faiss IndexShards
 *           (src/vod_search/faiss_search/server.py:51-54, src/vod_configs/search.py:80).
 * Shard g (on devices[g]; a device may be listed more than once) holds the global rows [g * R, (g + 1) * R), R = ceil(capacity /
 * n_devices): rows keep their insertion ids, the shards are balanced when the store is full.  A search replicates the query batch,
 * runs on every device at once, copies the per-shard top-k lists to devices[0] (peer copies) and merges them there with
 * vodhip_merge_topk: results are identical to one index holding all the rows.  (The Python host uses one process per GPU and one
 * RCCL all-gather instead - vod_amd/distributed.py - because that is how torch.distributed programs are launched.)
 *   add     HOST rows only (row-major [n_rows, dim] of src_dtype); the shards a batch straddles ingest concurrently; synchronous.
 *   search  location = VODHIP_HOST: queries / outputs are host buffers, the call returns with the results in place (`stream` unused);
 *           location = VODHIP_DEVICE: they live on devices[0]; the queries must be complete on `stream` and the outputs are complete
 *           on `stream` when the call returns (the exactness check of every shard has already been done on the host).
 *   shard   the per-device handle (for params, stats, subset labels, persistence), its id offset and its device.
 * Calls on one handle are serialised by the library (a mutex per handle); a search that fails half-way leaves no shard with a search
 * in flight.  `set_query_labels` + `search` are two calls: callers that filter from several threads go through a vodhip_batcher.
 * ------------------------------------------------------------------------------------------- */
typedef struct vodhip_node_index vodhip_node_index_t;
int vodhip_node_index_create(int n_devices, const int* devices, int64_t dim, int store_dtype, int64_t capacity_rows,
                             vodhip_node_index_t** out);
int vodhip_node_index_destroy(vodhip_node_index_t* index);
int vodhip_node_index_add(vodhip_node_index_t* index, const void* rows, int64_t n_rows, int src_dtype);
int vodhip_node_index_reset(vodhip_node_index_t* index);
int vodhip_node_index_ntotal(const vodhip_node_index_t* index, int64_t* out);
int vodhip_node_index_n_shards(const vodhip_node_index_t* index);
int vodhip_node_index_shard(vodhip_node_index_t* index, int g, vodhip_index_t** shard, int64_t* id_base, int* device);
int vodhip_node_index_set_param(vodhip_node_index_t* index, const char* key, int64_t value);  /* on every shard; plus "host_staging" (below) */
/* Topology, read once at create (hipDeviceCanAccessPeer both ways; peer access is enabled where possible): out[g] = 2 when shard g lives
 * on devices[0] itself, 1 when it exchanges with devices[0] by direct peer copies (xGMI), 0 when it goes through pinned host memory
 * (no peer access, or param "host_staging" = 1: every shard but the first takes that route - bring-up / tests on a 1-GPU box).
 * Returns the number of shards. */
int vodhip_node_index_peer_access(const vodhip_node_index_t* index, int* out, int n);
/* The subset filter of vodhip_index_set_row_labels / _set_query_labels behind the one handle: `labels` = HOST int32 [n_rows] for the
 * global rows 0 .. n_rows-1 (NULL clears); `q_labels` = int32 [nq, n_per_query] of the NEXT searches' batches, host memory or on
 * devices[0] (`location`), caller-owned until cleared with NULL; replicated to every device with the queries. */
int vodhip_node_index_set_row_labels(vodhip_node_index_t* index, const int32_t* labels, int64_t n_rows);
int vodhip_node_index_set_query_labels(vodhip_node_index_t* index, const int32_t* q_labels, int n_per_query, int location);
int vodhip_node_index_search(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, int k, int location,
                             float* out_scores, int64_t* out_ids, void* stream);
/* The same search in two halves (round 6), so that the host enqueues batch i + 1 on every shard while batch i runs - with 8 shards the
 * enqueue alone is ~0.3 ms of host time per batch: `search_async` replicates the queries and enqueues every shard's search (nothing is
 * waited for), `search_finish` completes the OLDEST pending search (every shard's exactness check, the lists' copies to devices[0], the
 * merge; HOST outputs are complete on return, DEVICE outputs on `stream`).  Up to 2 searches may be pending; queries, outputs and subset
 * labels of a pending search must stay valid until its finish.  `vodhip_node_index_search` = async + finish. */
int vodhip_node_index_search_async(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, int k, int location,
                                   float* out_scores, int64_t* out_ids, void* stream);
int vodhip_node_index_search_finish(vodhip_node_index_t* index);
/* H2i behind the one handle: queries, `ids` ([nq, m], GLOBAL row ids) and `q_labels` (may be NULL) are host buffers (location =
 * VODHIP_HOST) or live on devices[0]; so do the outputs.  The batch is replicated to every shard, every shard scores the whole list
 * into an aligned buffer of its own (rows of other shards are out of its range: -inf), the buffers meet on devices[0] and are combined
 * BY OWNERSHIP (owner = id / R; no comparison of values: a NaN survives), then ONE select runs for the top-k form: results equal one
 * index holding all the rows, bit for bit.  These calls synchronise with the host (the batch travels through host memory: listed
 * requests are small); DEVICE outputs are complete on `stream` on return, HOST outputs in place.  Serialised with the other calls on the
 * handle (its mutex); like a search, a call must not overlap add / reset / set_row_labels. */
int vodhip_node_index_score_ids(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, const int64_t* ids, int64_t m,
                                const int32_t* q_labels, int n_per_query, int location, float* out_scores, void* stream);
int vodhip_node_index_search_ids(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, const int64_t* ids, int64_t m,
                                 int k, const int32_t* q_labels, int n_per_query, int location, float* out_scores, int64_t* out_ids,
                                 void* stream);
/* H2w behind the one handle: `ids` ([nq, m], GLOBAL row ids), `weights` ([nq, m]), `q_labels` (may be NULL) and `out` ([nq, dim]) are
 * host buffers (location = VODHIP_HOST) or live on devices[0], under the rule of vodhip_node_index_score_ids.  The batch is replicated
 * to every shard; shard g runs vodhip_index_sum_ids with id_base = g * R, so that it sums the rows it owns (rows of other shards are
 * out of its range); the per-shard [nq, dim] sums meet on devices[0] and are added there in INCREASING SHARD ORDER.  The result is
 * deterministic for a given sharding; it need not be the flat index's bits (the association differs) and is where every sum is exact.
 * Host-synchronous (the batch travels through host memory); DEVICE outputs are complete on `stream` on return, HOST outputs in place.
 * Serialised with the other calls on the handle; refusals as for the flat call, and an invalid location. */
int vodhip_node_index_sum_ids(vodhip_node_index_t* index, const int64_t* ids, const float* weights, int64_t nq, int64_t m,
                              const int32_t* q_labels, int n_per_query, int location, float* out, void* stream);
/* H2p behind the one handle: queries, `q_labels` (may be NULL) and both outputs are HOST buffers.  Every shard runs
 * vodhip_index_log_partition on its own device and stream; the 2 * nq floats per shard return through host memory and are folded in
 * increasing shard order: max = max_g max_g, log_rel = log sum_g exp(beta (max_g - max) + log_rel_g); a shard with no eligible row
 * contributes nothing.  out_max equals one index holding all the rows bit for bit; out_log_rel within the rounding of the fold.
 * Host-synchronous; serialised with the other calls on the handle; refusals as for the flat call. */
int vodhip_node_index_log_partition(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                    const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                    float* out_max, float* out_log_rel /* HOST [nq] */);
/* H2t behind the one handle: HOST buffers, as above.  Every shard runs vodhip_index_posterior_stats; the 4 * nq floats per shard are
 * folded on the host in increasing shard order, in double (stats_fold.h): the pair as above; with w_g = exp(beta (max_g - max) +
 * log_rel_g - log_rel) and u_g = mean_rel_g + max_g - max, mean_rel = sum_g w_g u_g and var = max(0, sum_g w_g (var_g + u_g^2) -
 * mean_rel^2).  A shard with no eligible row carries weight 0; a folded maximum that is not finite gives NaN statistics. */
int vodhip_node_index_posterior_stats(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                      const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                      float* out_max, float* out_log_rel, float* out_mean_rel, float* out_var /* HOST [nq] each */);
/* H2d behind the one handle: HOST buffers, as above.  Every shard runs vodhip_index_posterior_divergence; the 8 * nq floats per shard
 * are folded on the host in increasing shard order, in double (divergence_fold.h): each side's pair and mean_rel as H2t's fold, and
 * cross_rel_ab = sum_g w^a_g (cross_rel_ab_g + max_b_g - max_b) with side a's weights.  A shard in which side a has mass and side b
 * no finite score gives -inf; a side whose folded maximum is not finite gives NaN for its mean_rel and for both cross words. */
int vodhip_node_index_posterior_divergence(vodhip_node_index_t* index, const void* queries_a, const void* queries_b, int q_dtype, int64_t nq,
                                           float beta_a, float beta_b, const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                           float* out_max_a, float* out_log_rel_a, float* out_mean_rel_a, float* out_cross_rel_ab,
                                           float* out_max_b, float* out_log_rel_b, float* out_mean_rel_b, float* out_cross_rel_ba /* HOST [nq] each */);
/* H2r behind the one handle: queries, ids / thresholds / tie ids, `q_labels` (may be NULL) and the outputs are HOST buffers; ids are
 * GLOBAL row ids.  rank_ids: every shard picks the scan scores of the ids it owns (vodhip_index_scan_score_ids with id_base = its
 * first global row), the host combines them by ownership - no values are compared -, every shard counts its rows against the combined
 * (score, global id) pairs (vodhip_index_count_above), and the host adds the counts in int64 (rank_fold.h).  count_above: the last two
 * steps alone.  Ranks, counts and scores equal one index holding all the rows bit for bit.  Host-synchronous; serialised with the
 * other calls on the handle; refusals as for the flat calls. */
int vodhip_node_index_rank_ids(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, const int64_t* ids, int64_t m,
                               const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                               int64_t* out_ranks, float* out_scores /* HOST [nq][m] */);
int vodhip_node_index_count_above(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, const float* thresholds,
                                  const int64_t* tie_ids /* HOST or NULL = strict */, int64_t m,
                                  const int32_t* q_labels /* HOST or NULL */, int n_per_query, int64_t* out_counts /* HOST [nq][m] */);
/* H2g behind the one handle: queries, thresholds, tie ids (GLOBAL row ids), `q_labels` (may be NULL), lims and the outputs are HOST
 * buffers.  Every shard runs vodhip_index_range_search with id_base = its first global row - the sizing call first, then, with outputs,
 * the full call - and the host concatenates a query's per-shard lists in shard order (range_fold.h): ascending ids, since shards own
 * ascending id ranges.  lims, scores and ids equal one index holding all the rows bit for bit.  lims[nq] > capacity: lims is complete,
 * positions below `capacity` are written, and the call returns an error that names both numbers.  Host-synchronous; serialised with the
 * other calls on the handle; refusals as for the flat call. */
int vodhip_node_index_range_search(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, const float* thresholds /* HOST [nq] */,
                                   const int64_t* tie_ids /* HOST [nq] or NULL = strict */, const int32_t* q_labels /* HOST or NULL */,
                                   int n_per_query, int64_t* lims /* HOST [nq + 1] */, float* out_scores /* HOST [capacity], or NULL */,
                                   int64_t* out_ids /* HOST [capacity], or NULL */, int64_t capacity);
/* H2m behind the one handle: HOST buffers, as above.  Every shard runs vodhip_index_posterior_mean; the shards are folded on the host
 * in increasing shard order, in double: the pair as above, mean = sum_g w_g mean_g with w_g = exp(beta (max_g - max) + log_rel_g -
 * log_rel); a shard with no eligible row carries weight 0 (its row is not read).  No eligible row anywhere, or a +inf score: zeros. */
int vodhip_node_index_posterior_mean(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                     const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                     float* out_max, float* out_log_rel /* HOST [nq] */, float* out_mean /* HOST [nq][dim] */);
/* H2e behind the one handle.  set_row_values: a HOST table [n_rows][n_cols] of src_dtype for the global rows (n_rows must equal ntotal;
 * NULL clears), split by shard row ranges - shard g keeps rows [g R, (g + 1) R) of it, a shard that holds no row a table of no rows;
 * reset drops it; rows added afterwards leave it short and the read-out is refused.  posterior_expectation: HOST buffers, as above.
 * Every shard runs vodhip_index_posterior_expectation; the shards are folded on the host in increasing shard order, in double
 * (readout_fold.h): the pair as H2p's fold, values = sum_g w_g values_g with w_g = exp(beta (max_g - max) + log_rel_g - log_rel); a
 * shard with no eligible row carries weight 0 (its rows are not read).  No eligible row anywhere, or a +inf score: zeros.  out_max
 * equals one index holding all the rows bit for bit.  Host-synchronous; serialised with the other calls on the handle; refusals as for
 * the flat calls. */
int vodhip_node_index_set_row_values(vodhip_node_index_t* index, const void* values /* HOST or NULL */, int64_t n_rows, int64_t n_cols,
                                     int src_dtype);
int vodhip_node_index_row_values_info(const vodhip_node_index_t* index, int64_t* n_rows, int64_t* n_cols);
int vodhip_node_index_posterior_expectation(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                            const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                            float* out_max, float* out_log_rel /* HOST [nq] */, float* out_values /* HOST [nq][n_cols] */);
/* H2b behind the one handle: HOST buffers, host-synchronous.  Every shard runs vodhip_index_posterior_expectation_backward on its own
 * rows with the GLOBAL (max_score, log_rel, values) of vodhip_node_index_posterior_expectation, so the shard results simply add: they
 * are folded on the host in increasing shard order, in double, and rounded once (readout_grad_fold.h).  Refusals as for the flat call. */
int vodhip_node_index_posterior_expectation_backward(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                                     const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                                     const float* max_score, const float* log_rel /* HOST [nq] */,
                                                     const float* values, const float* grad_values /* HOST [nq][n_cols] */,
                                                     float* out_grad_queries /* HOST [nq][dim] */);
/* H2a behind the one handle: HOST buffers, host-synchronous.  Every shard runs vodhip_index_posterior_adjoint on its own rows with the
 * GLOBAL (max_score, log_rel) it is handed (those of any node forward call), so shard g's result IS rows [g R, (g + 1) R) of the global
 * one: the slabs are concatenated (readout_adjoint_fold.h), nothing is folded.  Handed the words of one index holding all the rows, the
 * result equals that index's bit for bit.  `out` is overwritten (no accumulate).  Refusals as for the flat call. */
int vodhip_node_index_posterior_adjoint(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                        const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                        const float* max_score, const float* log_rel /* HOST [nq] */,
                                        const float* weights /* HOST [nq][n_cols] */, int64_t n_cols,
                                        float* out /* HOST [ntotal][n_cols] */);
/* H2k behind the one handle: HOST buffers, host-synchronous.  Every shard computes its own rows from the GLOBAL (max_score, log_rel,
 * values) and gradients it is handed.  The batch-wide scales are functions of those and of the table's column maxima: the node call
 * takes the largest of the shards' cached maxima - the maxima over all the rows - once and hands it to every shard, so each forms the
 * scales one index holding all the rows would (key_grad_fold.h).  The slabs are concatenated; nothing is folded.  Handed the words of
 * one index holding all the rows, the result equals that index's bit for bit.  `out` is overwritten (no accumulate).  Refusals as for
 * the flat call. */
int vodhip_node_index_posterior_key_gradient(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, float beta,
                                             const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                             const float* max_score, const float* log_rel /* HOST [nq] */,
                                             const float* grad_log_z /* HOST [nq], or NULL */,
                                             const float* values, const float* grad_values /* HOST [nq][n_cols], or NULL */,
                                             float* out /* HOST [ntotal][dim] */);
/* H2u behind the one handle: HOST ids (GLOBAL row ids, or NULL with the global row_begin) and HOST rows.  The call is ROUTED on the
 * host, not replicated (update_fold.h): the slots are partitioned by owning shard, id / rows_per_shard, in slot order - so the last
 * slot that lists a row is still the last its shard sees - and shard g receives its slots and their rows only, with id_base = its
 * first global row; the dense form splits at the shard boundaries.  A slot whose id is negative or not below ntotal goes to no shard
 * and is counted as skipped.  The shards are updated one after the other; the three stats of H2u are sums over the shards (+ those
 * slots) on vodhip_node_index_get_stat.  Refusals as for the flat call. */
int vodhip_node_index_update_rows(vodhip_node_index_t* index, const int64_t* ids /* HOST or NULL */, int64_t row_begin,
                                  const void* rows /* HOST */, int64_t n, int src_dtype, int mode, float alpha);
/* H2r behind the one handle: HOST ids (GLOBAL row ids, or NULL with the global row_begin).  Shard g owns the global ids
 * [g * rows_per_shard, (g + 1) * rows_per_shard) and vodhip_node_index_add fills the shards in order; removal restores that layout:
 * the slots are routed to their shards (update_fold.h; the range is split), every shard compacts locally with the flat call, then the
 * survivors are moved between the shards by an ordered list of segment copies, device to device, of every plane (remove_fold.h:
 * split at destination-shard boundaries, safe one after the other, an overlapping move inside one shard through its bounce buffer).
 * Afterwards the node index equals, byte for byte per shard, one freshly built from the survivors.  new_ids: HOST int64 [ntotal before
 * the call] of GLOBAL new ids, or NULL.  The three stats of H2r are sums over the shards on vodhip_node_index_get_stat (+ the slots
 * that no shard owns, skipped).  Host-synchronous.  Refusals as for the flat call. */
int vodhip_node_index_remove_rows(vodhip_node_index_t* index, const int64_t* ids /* HOST or NULL */, int64_t row_begin, int64_t n,
                                  int64_t* new_ids /* HOST [ntotal], or NULL */, int64_t* n_removed /* or NULL */);
/* H2s behind the one handle: HOST buffers, host-synchronous.  Every shard runs vodhip_index_sample_posterior with id_base = its first
 * global row; keys are unnormalised and the noise is a function of the global row, so the k + 1 best of the union of the shards'
 * lists ARE the k + 1 best of the whole store: ids, scores and keys equal one index holding all the rows bit for bit.  The pairs are
 * folded as above, the lists merged by (key desc, id asc) and log_p / log_weight recomputed in double from the folded pair
 * (sample_fold.h). */
int vodhip_node_index_sample_posterior(vodhip_node_index_t* index, const void* queries, int q_dtype, int64_t nq, int k, float beta,
                                       uint64_t seed, int64_t query_offset, const int32_t* q_labels /* HOST or NULL */, int n_per_query,
                                       float* out_max, float* out_log_rel /* HOST [nq] */, int64_t* out_ids, float* out_scores,
                                       float* out_log_p, float* out_log_weight /* HOST [nq][k] */, float* out_keys /* HOST [nq][k + 1] */);
/* With param "profile" = 1 (also set on every shard: their filter launches are bracketed, read per shard through vodhip_index_get_stat on
 * the handle vodhip_node_index_shard returns): "last_merge_ns" = the merge launch on devices[0], from the moment every shard's list had
 * arrived; "last_copy_ns_max" = the slowest shard's copy of its list towards devices[0] (peer copy over xGMI, or the down-leg to pinned
 * host memory when staged).  HIP events of the last search; 0 with one shard.  Waits for that search. */
int vodhip_node_index_get_stat(vodhip_node_index_t* index, const char* key, int64_t* out);

/* ---------------------------------------------------------------------------------------------
 * H4  hybrid score merge (lookup + up to VODHIP_MAX_ENGINES scored engines), one query row per wavefront.
 * Replaces: _merge_search_results (src/vod_dataloaders/core/search.py:79-125) =
 *           normalize_search_scores_ (core/normalize.py:6-20) + merge_search_results
 *           (core/merge.py:8-164) + gather_values_by_indices (core/numpy_ops.py:126-143).
 * All pointers are DEVICE pointers.  lookup_idx/lookup_lbl [nq, k_lookup] (lookup scores are discarded
 * by the reference, search.py:92).  engine e: idx[e] int64 [nq, k_e], scr[e] float32 [nq, k_e].
 * Outputs have `out_stride` = k_lookup + sum(k_e) + 1 columns allocated.  The reference cuts its buffer to
 * `[: max_cursor + 1]` after every pairwise fold (merge.py:160-162); out_width (device int32[VODHIP_MAX_ENGINES], may be
 * NULL) receives, per engine e, the maximum over rows of the cursor after engine e was folded in, from which the
 * caller derives the reference's final width: W = k_lookup; for e: W = min(out_width[e] + 1, W + k_e).
 * out_row_cursor (device int32 [nq, VODHIP_MAX_ENGINES], may be NULL) receives the same cursors per row with plain stores
 * (no cleared buffer, no atomics: one launch): vodhip_priority_sample_merged takes the maximum itself.
 *   out_idx  int64  : union of ids in first-seen order, -1 padded
 *   out_scr  float32: sum_e w_e * (s_e - rowmin_e), -inf padded
 *   out_lbl  int64  : lookup label of the id, -1 if absent (pad column: see SURVEY quirk Q3)
 *   out_raw[e] float32: min-subtracted score of the id in engine e, NaN if absent
 * ------------------------------------------------------------------------------------------- */
#define VODHIP_MAX_ENGINES 4
int vodhip_merge_hybrid(const int64_t* lookup_idx, const int64_t* lookup_lbl, int k_lookup,
                        int n_engines, const int64_t* const* engine_idx, const float* const* engine_scr,
                        const int* engine_k, const float* engine_weight, int64_t nq,
                        int64_t* out_idx, float* out_scr, int64_t* out_lbl, float* const* out_raw,
                        int out_stride, int32_t* out_width, int32_t* out_row_cursor, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H5  in-batch retrieval scoring + log-prob / loss combination, forward and backward fused.
 * Replaces: RetrievalGradients.__call__ (src/vod_models/vod_gradients/retrieval.py:30-92) with
 *           _compute_retriever_scores (:186-203), _cast_data_targets (:206-215), _compute_loss
 *           (:153-177), _compute_kld (:225-243) and the autograd backward of those.
 * q [B,H], s [D,H] (sections_3d = 0) or [B,D,H] (sections_3d = 1), of `enc_dtype` (F32 | F16 | BF16).
 * score/sparse/dense float32 [B,D] (sparse/dense may be NULL), relevance int64 [B,D].
 * Outputs (DEVICE): retriever_scores float32 [B,D]; d_scores float32 [B,D] (= dLoss/dScores);
 * loss float32 [1]; kl float32 [3] (score, sparse, dense; NaN where the input is NULL).
 * vodhip_retrieval_backward turns d_scores into dq [B,H] and ds ([D,H] | [B,D,H]) in float32,
 * scaled by *grad_out (device float32 scalar).
 * ------------------------------------------------------------------------------------------- */
int vodhip_retrieval_forward(const void* q, const void* s, int enc_dtype, int sections_3d,
                             int64_t B, int64_t D, int64_t H,
                             const float* score, const int64_t* relevance, const float* sparse, const float* dense,
                             float* retriever_scores, float* d_scores, float* loss, float* kl,
                             float* workspace /* DEVICE scratch, >= 8*B floats */, void* stream);
/* The same with the reference's auxiliary losses (RetrievalGradients._auxiliary_losses, retrieval.py:94-150):
 *   guidance          (weight > 0): huber(logp - ref) over entries finite in both, ref = sparse scores (guidance_type 1)
 *                                   or zeros (guidance_type 0)                                    (:116-126,180-183)
 *   self supervision  (weight > 0): cross entropy of the positives' log-probs against their own arg-max   (:129-140)
 *   score decay       (weight > 0): mean of the squared finite scores                                     (:143-145)
 * loss = KL term + sum(weight * term); d_scores carries every term's gradient.  aux_losses float32 [3] (DEVICE) receives the
 * three terms (NaN where the weight is 0); aux_grad is DEVICE scratch of 3*B*D floats (may be NULL when all weights are 0);
 * workspace holds workspace_floats >= 16*B floats; with >= 16*B + 4*B*D (2-D sections) the in-batch contraction is split over K
 * into slabs behind the row words and uses 4x the workgroups. */
int vodhip_retrieval_forward_aux(const void* q, const void* s, int enc_dtype, int sections_3d,
                                 int64_t B, int64_t D, int64_t H,
                                 const float* score, const int64_t* relevance, const float* sparse, const float* dense,
                                 int guidance_type, float guidance_weight, float self_supervision_weight, float score_decay,
                                 float* retriever_scores, float* d_scores, float* loss, float* kl, float* aux_losses,
                                 float* aux_grad, float* workspace /* DEVICE scratch */, int64_t workspace_floats, void* stream);
int vodhip_retrieval_backward(const void* q, const void* s, int enc_dtype, int sections_3d,
                              int64_t B, int64_t D, int64_t H, const float* d_scores, const float* grad_out,
                              float* dq, float* ds, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H5l marginal likelihood of a retrieval-augmented LM: fused token log-probs, marginal loss and every gradient.
 * Replaces: MarginalLikelihoodGradients.__call__ (src/vod_models/vod_gradients/marginal_likelihood.py:12-48) with
 *           _compute_lm_logprobs (:51-66: shift, masked_fill, log_softmax over V, gather, masked_fill, masked mean over L),
 *           _compute_retriever_scores (src/vod_models/vod_gradients/retrieval.py:186-203) and the autograd backward of those.
 * Three calls on one stream, split so that a caller can reuse the token log-probs; all pointers DEVICE, nothing synchronises.
 * lm_logits [N = B*D, L, V] contiguous, of `logits_dtype` (F32 | F16 | BF16), L >= 2, V and N*L below 2^31; input_ids int64 [N, L];
 * attention_mask [N, L] with elements of `mask_elem_bytes` (1 | 2 | 4 | 8) bytes, live when any bit is set.
 * Position t < L-1 of sequence n is LIVE when attention_mask[n, t+1] is; its target is input_ids[n, t+1].
 *   vodhip_lm_token_logprob_forward: tok_logp float32 [N, L-1] = logits[n,t,target] - logsumexp_v logits[n,t,:]; tok_lse float32
 *     [N, L-1, 2] = (row maximum, log sum exp(x - maximum)), kept for the backward.  Live rows are read once, 16 bytes per lane
 *     when V * element size is a multiple of 16 and the base is 16-byte aligned; masked positions write zeros, and neither
 *     their logits nor their ids are looked at.
 *   vodhip_marginal_forward: q [B,H], s [D,H] | [B,D,H] of `enc_dtype`, score float32 [B,D] (-inf = padded section).
 *     n = live positions of (b,d); lp_xz = sum of the live tok_logp / n; r = masked scores -> retriever_scores float32 [B,D];
 *     a = log_softmax_d(r) + lp_xz; loss float32 [1] = -mean_b logsumexp_d a; d_scores float32 [B,D] = dLoss/dr;
 *     coef float32 [B,D] = -exp(a - logsumexp_d a) / (B n).  workspace: workspace_floats >= B floats; with >= B + 4*B*D
 *     (2-D sections, H >= 512) the in-batch contraction is split over K into four slabs.  D <= 8192, and H + 3*D + 4 floats must fit 160 KiB.
 *     dq / ds follow from d_scores with vodhip_retrieval_backward.
 *   vodhip_lm_token_logprob_backward: d_logits [N, L, V] of `logits_dtype` = *grad_out * coef[n] * (1[v = target] - softmax_v)
 *     at live positions, exactly 0 at masked positions and at t = L-1: one read and one write of the tensor.
 * NaN rules (the reference raises an index error instead, which would need a host synchronisation): a LIVE target outside
 * [0, V-2] (the reference gathers from log_softmax(...)[..., :-1]) gives tok_logp = NaN, hence a NaN loss, with finite
 * retriever_scores; ids are compared before they index.  n = 0 gives NaN (0 / 0); a row whose sections are all padded gives
 * NaN.  -inf logits are legal, at the target too (that section then carries zero posterior; every gradient stays finite).
 * No atomics: two runs are bitwise equal.
 * ------------------------------------------------------------------------------------------- */
int vodhip_lm_token_logprob_forward(const void* lm_logits, int logits_dtype, int64_t N, int64_t L, int64_t V,
                                    const int64_t* input_ids, const void* attention_mask, int mask_elem_bytes,
                                    float* tok_logp, float* tok_lse, void* stream);
int vodhip_marginal_forward(const void* q, const void* s, int enc_dtype, int sections_3d,
                            int64_t B, int64_t D, int64_t H, const float* score, const float* tok_logp,
                            const void* attention_mask, int mask_elem_bytes, int64_t L,
                            float* retriever_scores, float* d_scores, float* coef, float* loss,
                            float* workspace /* DEVICE scratch */, int64_t workspace_floats, void* stream);
int vodhip_lm_token_logprob_backward(const void* lm_logits, int logits_dtype, int64_t N, int64_t L, int64_t V,
                                     const int64_t* input_ids, const void* attention_mask, int mask_elem_bytes,
                                     const float* tok_lse, const float* coef, const float* grad_out,
                                     void* d_logits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H5v the Renyi VOD objective over priority-sampled sections (Lievin et al., arXiv 2210.06345): the row stage between
 * vodhip_lm_token_logprob_forward and the two backward calls of H5 / H5l.
 * Replaces: nothing that runs - VodGradients is `raise NotImplementedError` in the reference (src/vod_models/vod_gradients/vod.py:14-26).
 * The quantity is the self-normalised importance-sampling estimate of the Renyi bound, differentiated as written with respect to
 * the model, the sampler held constant.  All pointers DEVICE, one stream, nothing synchronises.
 *   q [B,H], s [D,H] | [B,D,H] of `enc_dtype`; score, log_weight float32 [B,D] (section__score, -inf = padded section;
 *   section__log_weight, -inf = not sampled); log_proposal float32 [B,D] = the log proposal up to a per-row constant, or NULL:
 *   c = temperature * score.  tok_logp float32 [B*D, L-1] and attention_mask [B*D, L] as in H5l.
 *   A section is PADDED when score is -inf, and LIVE when it is not padded and neither log_weight nor c is -inf.  log_weight and
 *   c of a padded section are not looked at (c is not even formed: 0 * -inf).  Per query row, over its live set:
 *     r    = <q, s>                               -> retriever_scores float32 [B,D], -inf at padded sections (finite elsewhere,
 *                                                    live or not)
 *     n    = live positions of (b,d) ; l = sum of the live tok_logp / n (VODHIP_VOD_TOKEN_MEAN) | the sum (VODHIP_VOD_TOKEN_SUM)
 *     ls   = log_weight - logsumexp log_weight ; g = r - c ; lZ = logsumexp (ls + g) ; lw = l + g - lZ ; eps = 1 - alpha
 *     Lhat = sum exp(ls) lw                                                       (eps == 0: the ELBO)
 *          = m + log1p( sum exp(ls) expm1(eps (lw - m)) ) / eps                    (otherwise; continuous in float32 as alpha -> 1)
 *            for any shift m, max lw for one; the kernel takes m = logsumexp(ls + eps lw) / eps, the plain form of the same bound,
 *            so that the sum is ~ 0 and log1p does not magnify its rounding when the best section carries little weight
 *     omega = softmax (ls + eps lw) ; pi = softmax (ls + g)
 *   loss float32 [1] = -mean_b Lhat ; d_scores float32 [B,D] = -(omega - pi) / B ; coef float32 [B,D] = -omega / (B n) (MEAN) |
 *   -omega / B (SUM); both exactly 0 at every section that is not live, whose tokens and ids take no part.
 *   diag float32 [3] = mean_b of (Lhat at alpha = 0, Lhat at alpha = 1, 1 / sum omega^2): the importance-weighted bound, the ELBO
 *   and the effective sample size, from the same launch.  dq / ds follow from d_scores with vodhip_retrieval_backward, d_logits
 *   from coef with vodhip_lm_token_logprob_backward.
 * alpha (in [0, 1]), temperature (finite) and token_reduction are passed by value; eps is formed in double.
 * workspace: workspace_floats >= 4*B floats (the four row words); with >= 4*B + 4*B*D (2-D sections, H >= 512) the in-batch
 * contraction is split over K into four slabs.  D <= 8192, and H + 4*D + 4 floats must fit 160 KiB; what does not is refused.
 * NaN rules: a row without a live section gives a NaN loss (its gradients are 0).  NaN is not -inf: a NaN in log_weight or c of a
 * live section, n = 0 on a live section (both reductions) and, through tok_logp, a live target outside [0, V-2] of a live section
 * go through the formulas as written: the loss, the diagnostics and d_scores / coef of every live section of that row are NaN.  -inf logits at a target are legal: with eps > 0 that section gets omega = 0 and every gradient stays finite.
 * No atomics: two runs are bitwise equal.
 * ------------------------------------------------------------------------------------------- */
#define VODHIP_VOD_TOKEN_MEAN 0
#define VODHIP_VOD_TOKEN_SUM 1
int vodhip_vod_forward(const void* q, const void* s, int enc_dtype, int sections_3d,
                       int64_t B, int64_t D, int64_t H,
                       const float* score, const float* log_weight, const float* log_proposal /* may be NULL */,
                       const float* tok_logp, const void* attention_mask, int mask_elem_bytes, int64_t L,
                       double alpha, double temperature, int token_reduction,
                       float* retriever_scores, float* d_scores, float* coef, float* loss, float* diag,
                       float* workspace /* DEVICE scratch */, int64_t workspace_floats, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H5p sequence pooling of the encoder's last hidden state: aggregate, activation, norm and scale, fused, with backward.
 * Replaces: VodPooler.forward, MeanAgg, ClsAgg (src/vod_models/vod_encoder/modeling.py:76-89,164-174) and their autograd backward.
 * All pointers DEVICE, every call runs on `stream`, nothing synchronises, no atomics: two runs are bitwise equal.
 * hidden [N, L, H] contiguous of `hidden_dtype` (F32 | F16 | BF16); attention_mask [N, L] with elements of `mask_elem_bytes`
 * (1 | 2 | 4 | 8) bytes, live when any bit is set; N*L below 2^31, L >= 1, 1 <= H <= 2^30.  All arithmetic is float32.
 *   cnt[n] = live elements of mask row n; c = exp(0.5 * *log_scaler) (a float32 DEVICE word); eps = 1e-12.
 *   aggregate a float32 [N, H]:
 *     VODHIP_POOL_AGG_MEAN, VODHIP_POOL_MASK_REFERENCE: a = (sum over ALL L positions of hidden[n,l,:]) / cnt[n], the reference's
 *       arithmetic (padded positions are summed);  VODHIP_POOL_MASK_MASKED: a = (sum over the live positions) / cnt[n], padded token
 *       rows are not read.  cnt = 0 gives a = 0 in both.
 *     VODHIP_POOL_AGG_CLS: a = hidden[n,0,:]; the mask is ignored.
 *   finish on z (= a, or a projection of it, [N, P]): t = act(z) with VODHIP_POOL_ACT_* (gelu in its exact erf form);
 *     u = t (NORM_NONE) | t / max(|t|_2, eps) (NORM_L2) | t / max(|t|_1, eps) (NORM_L1); y = c u.
 *   vodhip_pool_forward: always writes a; with finish != 0 also y [N, H] of `y_dtype` (y may be NULL otherwise).  Token rows are
 *     read once, 16 bytes per lane when H * element size is a multiple of 16 and the base is 16-byte aligned.  L is cut into chunks
 *     of `l_chunk` tokens (0 = automatic, a function of (N, L, H) alone); with one chunk per row the call is ONE launch, with more
 *     the chunks leave float32 partial sums in `workspace` (vodhip_pool_workspace_floats(N, L, H, l_chunk) floats; 0 for one chunk,
 *     and CLS never needs any) and a second launch sums them in chunk order and runs the same finish routine: the same bits.
 *   vodhip_pool_backward: with finish != 0, g = dL/dy [N, H] of `g_dtype`, da is recomputed from the saved a:
 *       du = c g; l2, |t| > eps: dt = (du - u (u.du)) / |t|_2; l1, |t|_1 > eps: dt = (du - sign(t) (u.du)) / |t|_1; below eps:
 *       dt = du / eps; da = dt act'(a);  gy float32 [N] = sum_h g y (dL/dlog_scaler = 0.5 * sum_n gy[n]).
 *     with finish == 0, g IS da (gy is not written and may be NULL).
 *     d_hidden [N, L, H] of `hidden_dtype`, written exactly once: da[n] / cnt[n] at every position (MEAN, REFERENCE) or at the live
 *     ones (MEAN, MASKED), da[n] at l = 0 (CLS), exactly 0 elsewhere.  A MEAN row with cnt = 0 gets zeros (the reference: NaN).
 *   vodhip_pool_finish_forward / _backward: the finish alone on z [N, P] of `z_dtype`, behind a projection; dz of `dz_dtype`.
 * ------------------------------------------------------------------------------------------- */
#define VODHIP_POOL_AGG_MEAN 0
#define VODHIP_POOL_AGG_CLS 1
#define VODHIP_POOL_MASK_REFERENCE 0
#define VODHIP_POOL_MASK_MASKED 1
#define VODHIP_POOL_ACT_NONE 0
#define VODHIP_POOL_ACT_RELU 1
#define VODHIP_POOL_ACT_TANH 2
#define VODHIP_POOL_ACT_SIGMOID 3
#define VODHIP_POOL_ACT_GELU 4
#define VODHIP_POOL_NORM_NONE 0
#define VODHIP_POOL_NORM_L2 1
#define VODHIP_POOL_NORM_L1 2
int64_t vodhip_pool_workspace_floats(int64_t N, int64_t L, int64_t H, int64_t l_chunk); /* < 0: invalid sizes */
int vodhip_pool_forward(const void* hidden, int hidden_dtype, int64_t N, int64_t L, int64_t H,
                        const void* attention_mask, int mask_elem_bytes, int agg, int mask_mode,
                        int finish, int act, int norm, const float* log_scaler, int64_t l_chunk,
                        float* a, void* y, int y_dtype,
                        float* workspace /* DEVICE scratch */, int64_t workspace_floats, void* stream);
int vodhip_pool_backward(const void* g, int g_dtype, const float* a, int64_t N, int64_t L, int64_t H,
                         const void* attention_mask, int mask_elem_bytes, int agg, int mask_mode,
                         int finish, int act, int norm, const float* log_scaler, int64_t l_chunk,
                         void* d_hidden, int hidden_dtype, float* gy, void* stream);
int vodhip_pool_finish_forward(const void* z, int z_dtype, int64_t N, int64_t P, int act, int norm,
                               const float* log_scaler, void* y, int y_dtype, void* stream);
int vodhip_pool_finish_backward(const void* z, int z_dtype, const void* g, int g_dtype, int64_t N, int64_t P,
                                int act, int norm, const float* log_scaler,
                                void* dz, int dz_dtype, float* gy, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H5m retrieval metrics of the monitor that follows the loss: every (metric, topk) of one update in two launches.
 * Replaces: RetrievalMonitor.update (src/vod_models/monitoring/monitor.py:83-105) with prepare_for_metric_computation /
 *           _mask_rank_inputs (src/vod_models/monitoring/functional.py:15-25,164-178), the nine _compute_* functions
 *           (functional.py:41-161) and MeanAggregator.update (src/vod_models/monitoring/aggregator.py:43-50).
 * scores float32 [B, width] and relevances int64 [B, width] are DEVICE pointers, width <= 4096.  `specs` is a HOST array of
 * n_specs <= VODHIP_MAX_METRIC_SPECS pairs (metric, topk); topk = 0 means no cut.  Per row: n_positives = count(relevance > 0)
 * BEFORE masking; a NaN or +inf score becomes -inf with relevance 0; -inf is padding, ranked last and not masked; the row is
 * ranked by score descending, ties to the smaller column (-0.0 ranks as +0.0; the reference's argsort is unstable), cut at topk.
 *   MRR / HITRATE (0 or 1) / PRECISION (over the FINITE scores of the cut; 0/0 = NaN) / RECALL (over n_positives; 0/0 = NaN)
 *   NDCG: graded relevances / log2(rank + 1), the ideal order taken over the CUT list; 0 where the ideal DCG is 0
 *   KLDIV: log-softmax over the graded relevances of the cut's positives against log-softmax over its finite scores, summed
 *          where both are finite; NaN without a positive in the cut
 *   MIN / MAX over the finite scores of the cut (+inf / -inf without one)
 *   ENTROPY: -(exp(score) * log_softmax(score)) summed over the finite entries - exp of the SCORE, as the reference has it
 * values (DEVICE float32 [n_specs][B], may be NULL) receives the per-row values.  state (DEVICE float64 [n_specs][2], may be
 * NULL) is updated in place: state[m][0] += sum, state[m][1] += count of the non-NaN row values of spec m, reduced in a fixed
 * order (bit-reproducible).  With values == NULL the row values are kept in `workspace` (DEVICE, >= n_specs * B * 4 bytes).
 * Invalid arguments return a negative status before anything is launched.
 * ------------------------------------------------------------------------------------------- */
#define VODHIP_METRIC_MRR 0
#define VODHIP_METRIC_HITRATE 1
#define VODHIP_METRIC_PRECISION 2
#define VODHIP_METRIC_RECALL 3
#define VODHIP_METRIC_NDCG 4
#define VODHIP_METRIC_KLDIV 5
#define VODHIP_METRIC_MIN 6
#define VODHIP_METRIC_MAX 7
#define VODHIP_METRIC_ENTROPY 8
#define VODHIP_MAX_METRIC_SPECS 32
int vodhip_retrieval_metrics(const float* scores, const int64_t* relevances, int64_t B, int width,
                             const int32_t* specs /* HOST [n_specs][2]: metric, topk (0 = none) */, int n_specs,
                             float* values /* DEVICE [n_specs][B], may be NULL */,
                             double* state /* DEVICE [n_specs][2], += ; may be NULL */,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * H7  labeled priority sampling of the merged candidates (the collate stage right after the merge).  The *_proposal entry points
 *     below also emit the sampler's proposal (log_p per sample, the log-mass of each stratum, the joint weights): see there.
 * Replaces: _labeled_priority_sampling_2d_ / _labeled_priority_sampling_1d_ / _priority_sampling_1d
 *           (src/vod_dataloaders/core/sample.py:160-219,245-352) and the numba log-softmax helpers
 *           (src/vod_dataloaders/core/numpy_ops.py:162-216).
 * DEVICE pointers.  scores float32 [nq, width]; labels uint8 [nq, width] (non-zero = positive);
 * noise float32 [nq, width] = Exp(1) draws supplied by the caller (the reference draws them with
 * np.random.exponential on the host, sample.py:398), width <= 4096.
 * Outputs: samples int64 [nq, k_total] = column index into the row (-1 padded), log_weights float32
 * [nq, k_total] (-inf padded), out_labels uint8 [nq, k_total], lse float32 [nq, 2] (positives, negatives).
 * Reference quirks kept: support truncation masks entries >= the
 * `max_support_size`-th largest - it REMOVES the best entries of each class (src/vod_dataloaders/core/sample.py:176-178); ties in
 * the priority keys are broken by the smaller column.  `normalized` is a flag word: bit 0 = log-softmax the selected weights
 * (the reference's `normalized`), bit 1 = VODHIP_SAMPLE_KEEP_TOP_SUPPORT: the corrected truncation - KEEP the `max_support_size`
 * best entries of each class, mask the rest (what the parameter's name and the shipped `support_size: 100` intend).  Off by
 * default everywhere: bit parity with the reference is the default.
 * ------------------------------------------------------------------------------------------- */
#define VODHIP_SAMPLE_KEEP_TOP_SUPPORT 2
int vodhip_priority_sample(const float* scores, const uint8_t* labels, const float* noise, int64_t nq, int width,
                           int k_positive, int k_total, float temperature, int max_support_size, int normalized,
                           int64_t* out_samples, float* out_log_weights, uint8_t* out_labels, float* out_lse,
                           void* stream);

/* The same sampling, also emitting the sampler's PROPOSAL: what an importance-weighted objective over the samples (H5v,
 * vodhip_vod_forward) needs besides the per-stratum weights.
 * Replaces: nothing the reference returns - it forms these quantities and discards them (src/vod_dataloaders/core/sample.py:180-184,
 *           281-306): `log_norm_const` is taken AFTER log_softmax_1d_, so lse_pos / lse_neg above are ~0 and the share of each stratum
 *           in the row's mass is lost.
 * Per row, with a_i = t_inv * score_i (NaN -> -inf; after the support truncation) and a stratum S = the positives or the negatives:
 *   out_log_mass [nq, 2]            log_mass_S = logsumexp_{i in S} a_i (-inf for an empty or an all -inf stratum)
 *   out_log_proposal [nq, k_total]  log_p_j = a_j - log_mass_S(j): the float32 value the weight formula reads; -inf pad
 *   out_joint_log_weights [nq, k_total]  out_log_weights_j + log_mass_S(j) - logaddexp(log_mass_pos, log_mass_neg): the weights of
 *                                   ONE softmax over the whole row; -inf pad, -inf for a member of a stratum without mass.
 *                                   Needs bit 0 of `normalized` (an error before launch otherwise).
 * Each of the three may be NULL; with all three NULL the call writes the bits vodhip_priority_sample writes.  DEVICE pointers. */
int vodhip_priority_sample_proposal(const float* scores, const uint8_t* labels, const float* noise, int64_t nq, int width,
                                    int k_positive, int k_total, float temperature, int max_support_size, int normalized,
                                    int64_t* out_samples, float* out_log_weights, uint8_t* out_labels, float* out_lse,
                                    float* out_log_proposal, float* out_log_mass, float* out_joint_log_weights, void* stream);

/* The same sampling fed straight from vodhip_merge_hybrid's full-stride outputs, with the gathers and the rank diagnostic of
 * sample_search_results (src/vod_dataloaders/core/sample.py:22-84) as an epilogue: the collate's merge -> sample chain stays on
 * the device (reference flow src/vod_dataloaders/realm_collate.py:110-122).
 * DEVICE pointers.  ids int64 / scores float32 / labels int64 (> 0 = positive; the merge's lookup labels) / raw[e] float32, all
 * [nq, stride]; noise float32 rows of `noise_stride` elements.  `width` >= 0: the columns in use; `width` < 0: the reference's cut
 * (merge.py:160-162) is derived ON THE DEVICE from merge_width (the merge's out_width) or merge_row_cursor (its out_row_cursor;
 * one of the two), k_lookup and engine_k - no host sync between the two launches.  `raw` / `out_raw` are HOST arrays of n_raw (<= VODHIP_MAX_ENGINES) device pointers.
 * Outputs [nq, k_total]: out_samples (column index, -1 pad), out_ids / out_scores / out_raw[e] = take_along_axis by the sampled
 * columns (a -1 pad takes the LAST column in use, as NumPy does), out_log_weights, out_labels uint8; out_lse float32 [nq, 2];
 * out_max_sampling_id float32 [nq] = number of finite negatives of the pool scoring >= the lowest sampled finite negative. */
int vodhip_priority_sample_merged(const int64_t* ids, const float* scores, const int64_t* labels, int n_raw,
                                  const float* const* raw, const float* noise, int64_t noise_stride, int64_t nq, int stride,
                                  int width, const int32_t* merge_width, const int32_t* merge_row_cursor, int k_lookup,
                                  int n_engines, const int* engine_k,
                                  int k_positive, int k_total, float temperature, int max_support_size, int normalized,
                                  int64_t* out_samples, int64_t* out_ids, float* out_scores, float* out_log_weights,
                                  uint8_t* out_labels, float* const* out_raw, float* out_lse, float* out_max_sampling_id,
                                  void* stream);

/* vodhip_priority_sample_merged + the three proposal outputs of vodhip_priority_sample_proposal (same shapes, each may be NULL).
 * Replaces: see vodhip_priority_sample_proposal (src/vod_dataloaders/core/sample.py:180-184, 281-306). */
int vodhip_priority_sample_merged_proposal(const int64_t* ids, const float* scores, const int64_t* labels, int n_raw,
                                           const float* const* raw, const float* noise, int64_t noise_stride, int64_t nq, int stride,
                                           int width, const int32_t* merge_width, const int32_t* merge_row_cursor, int k_lookup,
                                           int n_engines, const int* engine_k, int k_positive, int k_total, float temperature,
                                           int max_support_size, int normalized, int64_t* out_samples, int64_t* out_ids,
                                           float* out_scores, float* out_log_weights, uint8_t* out_labels, float* const* out_raw,
                                           float* out_lse, float* out_max_sampling_id, float* out_log_proposal, float* out_log_mass,
                                           float* out_joint_log_weights, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gather by id: flattening of the sampled sections of a batch into ONE in-batch section set.
 * Replaces: gather_values_by_indices / gather_values_2d / _nopy_gather_values_{1d,2d}
 *           (src/vod_dataloaders/core/numpy_ops.py:24-143) as called by flatten_samples
 *           (src/vod_dataloaders/core/in_batch_negatives.py:10-52) for the scores, labels, log-weights and every
 *           raw engine score.
 * DEVICE pointers.  queries int64 [n_queries] (one id list shared by all rows: the sorted unique ids of the batch,
 * padded as the reference pads it); keys int64 [n_rows, n_keys] (n_keys <= 4096); `values` / `outs` are HOST arrays
 * of n_values (<= 8) DEVICE pointers to float32 [n_rows, n_keys] / [n_rows, n_queries]; fill[v] is written where
 * the id does not occur in the row (NaN for scores, 0 for labels in the reference).  First occurrence wins.
 * ------------------------------------------------------------------------------------------- */
int vodhip_gather_by_id(const int64_t* queries, int64_t n_queries, const int64_t* keys, int64_t n_rows, int n_keys,
                        int n_values, const float* const* values, const float* fill, float* const* outs, void* stream);

/* flatten_samples (src/vod_dataloaders/core/in_batch_negatives.py:10-52) in ONE launch: the sorted distinct ids of the whole
 * [n_rows, n_keys] batch, padded to U = n_rows * n_keys entries with the reference's constant 1 (out_unique int64 [U];
 * *out_n_unique = number of distinct ids, may be NULL), and every value array gathered onto that list (outs[v] float32
 * [n_rows, U], first occurrence wins, fill[v] where the row does not hold the id).  `labels` uint8 [n_rows, n_keys] (non-zero =
 * positive; may be NULL) is gathered the same way into out_labels uint8 [n_rows, U] with the reference's fill 0.
 * DEVICE pointers; `values` / `outs` HOST arrays of n_values (<= 8) device pointers.
 * Admitted shapes: U <= 8192, n_keys <= 1024, and the kernel's LDS (two id buffers of the whole batch + the row's 8 value arrays
 * and labels) within the 160 KiB of one workgroup.  Of the shapes inside the first two bounds the third excludes exactly
 * n_rows = 8 with n_keys = 1013 ... 1024 (8 rows hold at most 1012 ids each; 7 rows hold 1024).  Anything else is refused before
 * a launch: gather such a batch with vodhip_gather_by_id. */
int vodhip_flatten_inbatch(const int64_t* ids, int64_t n_rows, int n_keys, int n_values, const float* const* values,
                           const float* fill, float* const* outs, const uint8_t* labels, uint8_t* out_labels,
                           int64_t* out_unique, int32_t* out_n_unique, void* stream);

/* 1 when vodhip_flatten_inbatch (and the flattening step of vodhip_collate, n_rows = nq, n_keys = k_total) admits the shape, else 0:
 * the rule above, for callers that choose between the one-launch flattening and vodhip_gather_by_id.  No device work. */
int vodhip_flatten_inbatch_admits(int64_t n_rows, int n_keys);

/* ---------------------------------------------------------------------------------------------
 * The collate-side chain in ONE call: hybrid merge -> labeled priority sampling (+ gathers, rank diagnostic) -> optional
 * in-batch flattening = the three launches above enqueued back to back on `stream`, no host synchronisation.
 * Replaces the sequence RealmCollate.__call__ runs on the host (src/vod_dataloaders/realm_collate.py:110-139):
 *   _merge_search_results (core/search.py:79-125) -> sample_search_results (core/sample.py:22-84) -> flatten_samples
 *   (core/in_batch_negatives.py:10-52).
 * Every pointer is a DEVICE pointer owned by the caller.  stride = k_lookup + sum(engine_k) + 1 (n_engines >= 1).
 * ------------------------------------------------------------------------------------------- */
typedef struct vodhip_collate_args {
    /* the three engines' replies (core/search.py:42-62) */
    const int64_t* lookup_idx;                        /* [nq, k_lookup] */
    const int64_t* lookup_lbl;                        /* [nq, k_lookup] or NULL */
    const int64_t* engine_idx[VODHIP_MAX_ENGINES];    /* [nq, engine_k[e]] */
    const float* engine_scr[VODHIP_MAX_ENGINES];      /* [nq, engine_k[e]] */
    float engine_weight[VODHIP_MAX_ENGINES];
    int32_t engine_k[VODHIP_MAX_ENGINES];
    int32_t k_lookup, n_engines;
    int64_t nq;
    const float* noise;                               /* Exp(1) draws, rows of noise_stride >= stride elements (sample.py:398) */
    int64_t noise_stride;
    /* sampling parameters (sample_search_results' arguments) */
    int32_t k_positive, k_total, max_support_size, in_batch_negatives;
    float temperature;
    int32_t flags;                                    /* 0, or VODHIP_SAMPLE_KEEP_TOP_SUPPORT */
    /* workspace: the merged rows at full stride (also an output: what _merge_search_results returns, uncut) */
    int64_t* merged_idx;                              /* [nq, stride] */
    int64_t* merged_lbl;                              /* [nq, stride] */
    float* merged_scr;                                /* [nq, stride] */
    float* merged_raw[VODHIP_MAX_ENGINES];            /* [nq, stride] each */
    int32_t* row_cursor;                              /* [nq, VODHIP_MAX_ENGINES] */
    /* sampled sections [nq, k_total] */
    int64_t* out_local;                               /* column of the merged row, -1 pad */
    int64_t* out_ids;
    float* out_scores;
    float* out_log_weights;
    uint8_t* out_labels;
    float* out_raw[VODHIP_MAX_ENGINES];
    float* out_lse_pos;                               /* [nq] */
    float* out_lse_neg;                               /* [nq] */
    float* out_max_sampling_id;                       /* [nq] */
    /* flattened batch (in_batch_negatives != 0): U = nq * k_total; the shape (nq, k_total) must be one vodhip_flatten_inbatch admits
     * (U <= 8192, k_total <= 1024, not 8 x 1013 ... 1024) - refused before anything is launched otherwise */
    int64_t* flat_ids;                                /* [U] */
    float* flat_scores;                               /* [nq, U] */
    float* flat_log_weights;                          /* [nq, U] */
    uint8_t* flat_labels;                             /* [nq, U] */
    float* flat_raw[VODHIP_MAX_ENGINES];              /* [nq, U] each */
    int32_t* flat_n_unique;                           /* [1] or NULL */
} vodhip_collate_args_t;
int vodhip_collate(const vodhip_collate_args_t* args, void* stream);

/* vodhip_collate + the sampler's proposal (vodhip_priority_sample_proposal has the definitions): merge -> sample -> (flatten) then
 * feeds the VOD objective with no host work.  Two exact ways to feed it: "stratum" = out_log_weights as section__log_weight and
 * out_log_proposal as section__log_proposal; "joint" = out_joint_log_weights as section__log_weight and no proposal (the objective's
 * temperature must then be the sampler's).
 * Replaces: what the reference discards in src/vod_dataloaders/core/sample.py:180-184, 281-306.
 * `base` is the argument block of vodhip_collate, unchanged, at offset 0.  Every new pointer is a DEVICE pointer and may be NULL;
 * with all of them NULL the call is vodhip_collate(&args->base, stream).  The flattened arrays fill with -inf (not NaN) where a
 * row did not sample the id; each needs its [nq, k_total] source output and base.in_batch_negatives.  Same stream, same launches. */
typedef struct vodhip_collate_proposal_args {
    vodhip_collate_args_t base;
    float* out_log_proposal;                          /* [nq, k_total] */
    float* out_log_mass_pos;                          /* [nq] (with out_log_mass_neg, or both NULL) */
    float* out_log_mass_neg;                          /* [nq] */
    float* out_joint_log_weights;                     /* [nq, k_total] */
    float* flat_log_proposal;                         /* [nq, U] */
    float* flat_joint_log_weights;                    /* [nq, U] */
} vodhip_collate_proposal_args_t;
int vodhip_collate_proposal(const vodhip_collate_proposal_args_t* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Wire codec helper (HOST memory, no device work): urlsafe base64 of `head || data` and back.
 * Replaces the inner loops of: serialize_np_array / deserialize_np_array (src/vod_search/io.py:17-32:
 *   base64.urlsafe_b64encode(np.save(...)) / np.load(base64.urlsafe_b64decode(...))), which cost ~9 ms per
 *   direction for a 1024 x 768 float32 batch in CPython; output is byte-identical ('-' '_' alphabet, '=' padding).
 * encode: writes 4*ceil((n_head+n_data)/3) chars to `out`, returns that count.
 * decode: accepts both alphabets, stops at '=' padding; returns the number of bytes written to `out`
 *         (capacity >= 3*n/4), or -1 if a character outside the alphabets is met (the caller falls back to
 *         the lenient library decoder) - never reads or writes out of bounds.
 * ------------------------------------------------------------------------------------------- */
int64_t vodhip_b64url_encode(const uint8_t* head, int64_t n_head, const uint8_t* data, int64_t n_data, char* out);
int64_t vodhip_b64url_decode(const char* src, int64_t n, uint8_t* out);

/* ---------------------------------------------------------------------------------------------
 * H6  serving: request fusion in front of one index + an HTTP/1.1 front for the search service's hot routes
 *     (host code only; native threads, no interpreter on the request path).
 * Replaces: the reference's single uvicorn worker, which runs `faiss_index.search` for ONE request at a time
 *           (src/vod_search/faiss_search/server.py:57-98) while every DataLoader worker of every trainer rank sends its own small
 *           batch (src/vod_dataloaders/realm_dataloader.py:92-118, core/search.py:128-146); and the wire codec of
 *           src/vod_search/io.py:17-32 on the server side of /fast-search.
 *
 * vodhip_batcher   fuses concurrent searches into shared corpus scans (a brute-force scan reads the whole store whatever the batch
 *   size).  Exactly one engine: `index` (searches are pipelined on the batcher's own stream, up to "depth" batches on the device,
 *   result rows written straight into device-visible host memory), `node` (the node index; two batches in flight since round 6: vodhip_node_index_search_async / _finish) or `fn` (a host
 *   callback `fn(user, float32 queries [nq, dim], nq, k, subset | NULL, n_subset, out_scores, out_ids) -> 0 | error`, e.g. a
 *   multi-process group; needs no GPU in this process).  The batcher OWNS the engine's search path while it exists: do not call
 *   vodhip_index_search* on the same handle from elsewhere.
 *   search: blocking, thread-safe; host pointers; q_dtype F32 | F16 (| BF16 for index / node); `subset` = int32 [nq, n_subset]
 *     allowed row labels (vodhip_index_set_query_labels semantics; such a request runs as its own batch) or NULL; `client` = a tag
 *     of the requester (connection id; 0 = anonymous).  Results are identical to separate vodhip_index_search calls: the fused batch
 *     runs with k = max(k_i) and a prefix of a top-k' list is the top-k.
 *   policy (no fixed wait window): a request that finds the engine idle runs at once, unless other clients that searched a moment
 *     ago have nothing pending yet and the batch still fits one query tile ("flat_queries", 256: the scan costs the same with them
 *     aboard) and are DUE (their usual come-back time after an answer, an EMA per client, ends before the grace does) - then it waits for
 *     them at most min("grace_us", "grace_pct" % of a measured scan); requests that arrive while a batch
 *     is on the device are fused, and enqueued behind it once they exceed one query tile (time is linear from there) or when it
 *     completes.  params: "max_queries" (2048), "flat_queries", "grace_us" (1000; 0 = never wait), "grace_pct" (35), "window_us"
 *     (0; > 0 = additionally wait this long for company, round 3's --micro-batch-wait-ms), "depth" (2).
 *   stats: "batches", "requests", "queries", "fused_requests_max", "grace_waits", "grace_expired", "idle_ns", "busy_ns",
 *     "last_batch_queries", "last_batch_requests", "flat_scan_ns", "in_flight", "pending", "active_clients".
 * ------------------------------------------------------------------------------------------- */
typedef struct vodhip_batcher vodhip_batcher_t;
typedef int (*vodhip_search_fn)(void* user, const float* queries, int64_t nq, int k, const int32_t* subset, int n_subset,
                                float* out_scores, int64_t* out_ids);
int vodhip_batcher_create(vodhip_index_t* index, vodhip_node_index_t* node, vodhip_search_fn fn, void* user, int64_t dim,
                          int64_t id_base, vodhip_batcher_t** out);
int vodhip_batcher_destroy(vodhip_batcher_t* batcher);
int vodhip_batcher_set_param(vodhip_batcher_t* batcher, const char* key, int64_t value);
int vodhip_batcher_get_stat(vodhip_batcher_t* batcher, const char* key, int64_t* out);
int vodhip_batcher_search(vodhip_batcher_t* batcher, const void* queries, int q_dtype, int64_t nq, int k, const int32_t* subset,
                          int n_subset, uint64_t client, float* out_scores, int64_t* out_ids);
int vodhip_batcher_forget_client(vodhip_batcher_t* batcher, uint64_t client);  /* the requester went away (connection closed) */

/* vodhip_http  HTTP/1.1 server, one native thread per (keep-alive) connection, in front of a batcher:
 *   POST /fast-search  {"vectors": "<urlsafe-b64(np.save(float32|float16 [nq, dim]))>", "top_k": K}
 *                      -> {"scores": "<b64(npy f32 [nq, K])>", "indices": "<b64(npy i64 [nq, K])>"}   (server.py:76-91, io.py:17-32;
 *                      reply bytes identical to the reference's FastSearchResponse as this package's Python shell writes it)
 *   POST /raw-search?top_k=K   body = raw .npy bytes -> scores f32 [nq, K] || ids i64 [nq, K], shapes in x-nq / x-k
 *   GET  /stats        batcher + front counters as JSON (not in the reference)
 * are parsed, decoded, searched and encoded natively WHEN the request is the plain hot case (known keys, escape-free payload, version
 * 1.0 C-order 2-D .npy of the index dimension, 1 <= top_k <= VODHIP_MAX_K, no subset filter).  Every other request - GET /, POST
 * /search, subset filters, unknown fields, malformed payloads, out-of-range top_k - is handed unchanged to `fallback`, which answers
 * through vodhip_http_reply_set (status, content type, payload, extra "name: value\r\n" header lines): validation and error mapping
 * (422 / 500 + trace, models.py:43-79, server.py:89-91) live in ONE place, the host's.  `fallback` is called on the connection's
 * thread; NULL answers 404.  listen_tcp binds every address `host` resolves to and returns the port (port 0 = pick one);
 * start spawns the accept thread and returns; stop closes listeners and connections and waits for the connection threads. */
typedef struct vodhip_http vodhip_http_t;
typedef struct vodhip_http_reply vodhip_http_reply_t;
typedef void (*vodhip_http_fallback_fn)(void* user, const char* method, const char* target, const uint8_t* body, int64_t n_body,
                                        uint64_t client, vodhip_http_reply_t* reply);
int vodhip_http_reply_set(vodhip_http_reply_t* reply, int status, const char* content_type, const uint8_t* payload, int64_t n,
                          const char* extra_headers);
int vodhip_http_create(vodhip_batcher_t* batcher, int64_t dim, vodhip_http_fallback_fn fallback, void* user, int64_t max_body_bytes,
                       vodhip_http_t** out);
int vodhip_http_listen_tcp(vodhip_http_t* http, const char* host, int port);
int vodhip_http_listen_unix(vodhip_http_t* http, const char* path);
int vodhip_http_start(vodhip_http_t* http);
int vodhip_http_stop(vodhip_http_t* http);
int vodhip_http_destroy(vodhip_http_t* http);
int vodhip_http_get_stat(vodhip_http_t* http, const char* key, int64_t* out);  /* "requests_native", "requests_fallback", "connections", "open_connections" */

/* vodhip_client  the CLIENT side of the search service: one kept-alive HTTP/1.1 connection (TCP, or a Unix-domain socket when `unix_path`
 * is given) that speaks POST /fast-search - the reference's documents, byte for byte what its client sends and parses - and POST
 * /raw-search.  Replaces: FaissClient.search (src/vod_search/faiss_search/client.py:64-110) + io.serialize_np_array /
 * deserialize_np_array (src/vod_search/io.py:17-32) for consumers that are not Python (cgo / JNI: same C-ABI as the in-process index) and
 * for Python workers (one call with the GIL released instead of ~150 us of interpreter per exchange).
 *   One handle = one connection = one caller at a time (a handle per thread).  A connection the server closed while idle is re-opened once.
 *   search: queries host [nq, dim] F32 | F16; route 0 = /fast-search, 1 = /raw-search; timeout_s <= 0 = 120 s.
 *           returns 0 with out_scores / out_ids [nq, k] filled; > 0 = the HTTP status of an error reply (its body: vodhip_client_last_body -
 *           the server's `{"detail": ...}`); -1 = transport / protocol failure (vodhip_last_error; "timed out ..." for a timeout). */
typedef struct vodhip_client vodhip_client_t;
int vodhip_client_create(const char* host, int port, const char* unix_path, vodhip_client_t** out);
int vodhip_client_destroy(vodhip_client_t* client);
int vodhip_client_search(vodhip_client_t* client, const void* queries, int q_dtype, int64_t nq, int64_t dim, int k, int route, double timeout_s,
                         float* out_scores, int64_t* out_ids);
const char* vodhip_client_last_body(vodhip_client_t* client);

/* The native front's wire pieces, exposed so that they can be checked byte for byte against NumPy / the Python codec without a
 * socket or a GPU (tests/test_host_logic.py):
 *   npy_header         np.lib.format.write_array_header_1_0 for a C-ordered [rows, cols] array; dtype VODHIP_F32 | VODHIP_F16 | 3 (int64);
 *                      out >= 192 bytes; returns the header length (the data offset)
 *   parse_npy          0 + dtype / rows / cols / data offset for a version-1.0 little-endian float32 | float16 | int64 (dtype code 3)
 *                      C-order 2-D array whose data is complete; -1 for anything else (not an error: the host's reader takes over)
 *   parse_fast_search  0 + the [begin, end) span of the "vectors" payload and top_k (default 3) for the plain hot document; 1 otherwise
 *   fast_search_reply  the /fast-search reply body; out = NULL returns the size needed */
int64_t vodhip_wire_npy_header(int dtype, int64_t rows, int64_t cols, uint8_t* out, int64_t cap);
int vodhip_wire_parse_npy(const uint8_t* data, int64_t n, int* dtype, int64_t* rows, int64_t* cols, int64_t* data_offset);
int vodhip_wire_parse_fast_search(const char* body, int64_t n, int64_t* vec_begin, int64_t* vec_end, int64_t* top_k);
int64_t vodhip_wire_fast_search_reply(const float* scores, const int64_t* ids, int64_t nq, int k, char* out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* VODHIP_H */
