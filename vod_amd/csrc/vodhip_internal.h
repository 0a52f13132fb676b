// Internal declarations shared by the kernel translation units and the C-ABI layer of libvodhip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "search_plan.h"

// Diagnostic builds (`make ABLATION=1`): phase stamps of workgroup 0 of the collate-side kernels - shader-clock cycles
// (s_memtime) and the constant 100 MHz counter (s_memrealtime) - read back with vodhip_debug_read_probe.  Nothing in production.
#ifdef VODHIP_ABLATION
#define VODHIP_PROBE(buf, i)                                                  \
    do {                                                                      \
        if (blockIdx.x == 0 && threadIdx.x == 0) {                            \
            (buf)[2 * (i)] = (long long)__builtin_amdgcn_s_memtime();         \
            (buf)[2 * (i) + 1] = (long long)__builtin_amdgcn_s_memrealtime(); \
        }                                                                     \
    } while (0)
// begin / end stamp of EVERY workgroup (blocks 0..63 of the launch): buf[128 + 2 * block] = begin tick, + 1 = end tick
#define VODHIP_PROBE_WG(buf, end)                                                                                   \
    do {                                                                                                            \
        if (blockIdx.x < 64 && threadIdx.x == 0) (buf)[128 + 2 * blockIdx.x + (end)] = (long long)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define VODHIP_PROBE_WG(buf, end) \
    do {                          \
    } while (0)
#define VODHIP_PROBE(buf, i) \
    do {                     \
    } while (0)
#endif

namespace vodhip {

void set_last_error(const char* msg);  // the calling thread's vodhip_last_error() text (vodhip_node.hip composes public entry points)

// the index kinds no whole-store scan accepts, as the flat and the node entry points refuse them; %s = the operation's name
constexpr const char* SCAN_REFUSES_L2 = "%s is not supported on an L2 index (VODHIP_L2): its scores are distances, not similarities";
constexpr const char* SCAN_REFUSES_EXACT_F32 =
    "%s is not supported on a VODHIP_EXACT_F32 store: the scan scores the rounded rows, that store's contract is the float32 rows";

// which: 0 = merge_hybrid_kernel, 1 = priority_sample_kernel, 2 = flatten_inbatch_kernel; out: 256 words = 64 (cycles, 10 ns ticks) phase pairs + 64 (begin, end) workgroup pairs
hipError_t read_probe_hybrid(long long* out);
hipError_t read_probe_sample(int which, long long* out);
hipError_t read_probe_select(long long* out);  // which = 3: mips_select_kernel (final | threshold-only | middle launch at [0], [8], [16])

// 64-bit order-preserving result key: high 32 bits = monotone image of the fp32 score, low 32 bits =
// 0xFFFFFFFF - local row id.  Larger key == better hit (higher score; on equal score the smaller id).
// Key 0 is reserved for "no entry" and sorts below every real key.
typedef unsigned long long key_t64;

// Per-query candidate counters sit one per 128-byte line: every survivor is one returning atomic on its query's counter, and
// atomics on one line execute one after the other at the memory side (~3 ns each) - with the counters packed (8-32 lines for
// 256-1024 queries) the ~800 k atomics of a stage took 70 us whatever the stage's size (measured: a 166 k-row stage at
// nq = 256 ran 143 us with survivors, 74 us without).
constexpr int CNT_STRIDE = 32;  // in unsigned ints

enum : int { FILTER_FLAG_CORPUS_NT = 1 };  // FilterExtra::flags bit 0; bits 8.. = timing knobs of diagnostic builds

// Extra, optional inputs of the filter kernels (passed by value).
struct FilterExtra {
    int flags = 0;                    // FILTER_FLAG_* | (diagnostic knobs << 8)
    const int* row_label = nullptr;   // [ntotal] subset label of every stored row, or NULL (no subset filtering)
    const int* q_label = nullptr;     // [nq, n_qlab] allowed labels per query (-1 = empty slot; all -1 = unrestricted)
    int n_qlab = 0;
    int sample_rstride = 0;           // GMAX launches: store rows between consecutive sampled rows (>= 1)
    int sample_offset = 0;            // GMAX launches: first sampled row (centres the sample: the unsampled rows split between head and tail)
    int sample_groups = 0;            // GMAX launches: number of lane groups of the sample (= candidate slots per query)
    const int* q_map = nullptr;       // recovery of a few queries: workspace row -> row of the caller's batch (q_label is indexed by the latter)
    // FILTER launches: the order in which a search's stages walk the store's 256-row super-tiles.  perm_mod = T > 0: position p of the
    // sequence is super-tile (p * perm_mul) % T (perm_mul ~ 0.618 T, coprime to T: a low-discrepancy order - ANY run of consecutive
    // positions, i.e. any stage, is spread evenly over the whole store, so its threshold is calibrated on every topic of a
    // document-ordered corpus and a hot topic's tiles are not all scanned at once); 0 = positions are tiles.  row_bound = ntotal (the
    // partly filled last super-tile can sit at any position: every launch masks rows >= row_bound).
    int perm_mul = 0, perm_mod = 0, row_bound = 0;
};

struct SearchWorkspace {
    uint16_t* q_pad = nullptr;       // [nq_pad][dim_pad] queries rounded to the store dtype, zero padded
    key_t64* topk = nullptr;         // [nq_pad][kp] running top-k keys, sorted descending
    key_t64* cand = nullptr;         // [nq_pad][cap] candidate keys appended by the filter kernel
    unsigned int* cnt = nullptr;     // [nq_pad * CNT_STRIDE] candidates appended in the current stage (one counter per 128-B line)
    float* thr_s = nullptr;          // [nq_pad] score of the current k-th best (-inf until k hits exist)
    key_t64* thr_key = nullptr;      // [nq_pad] key of the current k-th best (0 until k hits exist)
    unsigned int* overflow = nullptr;  // [4] flag words: [0] a candidate buffer overflowed; exact mode: [1] some list did not prove complete, [2] max needed list length; [3] blocks that missed the 8-phase kernel's survivor rings
    unsigned int* ovf_q = nullptr;     // [nq] per query: its candidate list overflowed in some stage (set by the select kernel), or NULL
    // the 8-phase FILTER kernel's per-wave survivor rings (kernels_mips_8phase.hip): [waves][ring_cap][32] sums, then [waves][ring_cap]
    // metadata words, waves = 8 x the launch's grid; grow-only, `ring_floats` floats allocated
    float* ring = nullptr;
    int64_t ring_floats = 0;
    int64_t ring_cap = 0;              // records per wave of the search being enqueued (SearchPlan::ring; 0: no ring)
    int n_cu = 256;                    // compute units of the device (read once at index create)
    int64_t nq_cap = 0;
    int64_t cap = 0;
    int64_t kp = 0;       // row stride of `topk` for the search being enqueued (a power of two >= its k)
    int64_t kp_cap = 0;   // ... and the stride the buffer was allocated for (>= kp)
    FilterExtra extra;  // flags + optional subset filter of the current search
};

// ---- launchers (kernels_mips.hip) -------------------------------------------------------------
// store_dtype: 0 = f16, 1 = bf16.  kernel: the filter kernel (search_plan.h: the planner picks it per stage).
// mode: 0 = FILTER (threshold survivors -> candidate lists), 1 = DENSE (every score of rows [row_begin, row_end) is a
// candidate), 2 = GMAX (threshold bootstrap: group maxima of `n_sample_tiles` sampled tiles, see FilterExtra::sample_rstride).
hipError_t launch_convert_rows(const void* src, int src_dtype, int64_t n_rows, int64_t dim, void* dst, int dst_dtype,
                               int64_t dst_stride, hipStream_t stream);
// seed_scores / seed_ids ([nq, k] device, or NULL): a previous valid-but-incomplete result whose k-th score seeds the thresholds
// q_map ([nq] device, or NULL): workspace row r is row q_map[r] of q_src / of the seed arrays
// seed_margin ([rows of the caller's batch] device, or NULL): subtracted from the seeding score (the BAND pass of exact mode seeds
// its scan thresholds with `k-th exact score - eps`)
hipError_t launch_search_prepare(const SearchWorkspace& ws, const void* q_src, int q_dtype, int64_t nq, int64_t dim,
                                 int store_dtype, int64_t nq_pad, int64_t dim_pad, bool clear_overflow,
                                 const float* seed_scores, const int64_t* seed_ids, int k, const int* q_map, hipStream_t stream,
                                 const float* seed_margin = nullptr);
// flags: 1 = final (sort; the top-k also leaves as float32 scores / int64 ids (+ id_base) in out_scores / out_ids [nq, k]),
//        2 = threshold only (the candidates are GMAX group maxima: nothing enters the running top-k)
//        q_map: result row r is written to row q_map[r] of out_scores / out_ids
hipError_t launch_select(const SearchWorkspace& ws, int64_t nq, int k, int64_t dense_n, int flags, hipStream_t stream,
                         int64_t id_base = 0, float* out_scores = nullptr, int64_t* out_ids = nullptr, const int* q_map = nullptr);
hipError_t launch_output(const SearchWorkspace& ws, int64_t nq, int k, int64_t id_base, float* out_scores,
                         int64_t* out_ids, hipStream_t stream);
hipError_t launch_merge_topk(const float* scores, const int64_t* ids, int64_t stride_s, int64_t stride_i, int n_shards,
                             int64_t nq, int k, int k_out, float* out_scores, int64_t* out_ids, hipStream_t stream);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel): it is a driver call on the launch path
hipError_t allow_dynamic_lds(const void* kernel, int bytes);
// the FILTER stage on the guide's 8-phase K loop (kernels_mips_8phase.hip); lead / keep_b0 other than 7 / true: experiment builds only
hipError_t launch_filter_8phase(int store_dtype, int lead, bool keep_b0, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin,
                                int64_t row_end, int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream);
// A FILTER stage on the kernel of an experiment id (experiment_filter).
using FilterStageFn = hipError_t (*)(int store_dtype, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin, int64_t row_end,
                                     int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream);
// When t.tile is an experiment id: its FILTER kernel, and t becomes what the search plans with (the persistent kernel); else nullptr.
#ifdef VODHIP_EXPERIMENTS
FilterStageFn experiment_filter(PlanTunables& t);  // experiments/csrc/experiment_filter.hip
#else
inline FilterStageFn experiment_filter(PlanTunables&) { return nullptr; }
#endif
// experiment: the FILTER kernel of an experiment id (experiment_filter) that FILTER stages run instead of `kernel`, or nullptr
hipError_t launch_filter(int store_dtype, FilterKernel kernel, int mode, const void* store, const void* q_pad, int64_t dim_pad,
                         int64_t row_begin, int64_t row_end, int64_t n_sample_tiles, int64_t nq, int64_t nq_pad,
                         const SearchWorkspace& ws, hipStream_t stream, FilterStageFn experiment = nullptr);

// ---- launchers (kernels_exact.hip): the float32 plane of VODHIP_EXACT_F32 stores ----------------
enum : int { EXACT_LIST = 0, EXACT_CAND = 1, EXACT_FIRST = 2 };
struct ExactArgs {
    const float* plane = nullptr;     // [rows][stride] float32 rows (zero padded columns)
    int64_t stride = 0;
    int dim = 0, dim_pad = 0;
    const void* q_src = nullptr;      // the caller's queries [batch rows, dim] of q_dtype (unrounded)
    int q_dtype = 0;
    const int* q_map = nullptr;       // workspace row -> row of the caller's batch, or NULL
    int store_dtype = 0;              // what the scan rounded to (the bound needs |q - q~|)
    // the bound's statistics, host copies (refreshed before the first search after rows were added: launch_exact_stats)
    float ord_n2 = 0.f, ord_d2 = 0.f;     // max |x|^2, max |x - x~|^2 over the ORDINARY rows
    float cut_n2 = 0.f, cut_d2 = 0.f;     // a row with |x|^2 > cut_n2 or |x - x~|^2 > cut_d2 is an OUTLIER: scored by every query, not bounded
    int n_out = 0;                        // outliers (<= 2 * EXACT_MAX_OUTLIERS)
    const unsigned int* out_rows = nullptr;  // [n_out] their local rows (device)
    const float* row_n2 = nullptr;        // [rows] |x|^2 of every stored row (device)
    const float* row_d2 = nullptr;        // [rows] |x - x~|^2
    const int* row_label = nullptr;       // the subset filter in force (outliers are injected past the scan: they are filtered here), or NULL
    const int* q_label = nullptr;         // [batch rows, n_qlab]
    int n_qlab = 0;
    int mode = EXACT_LIST;            // EXACT_LIST | EXACT_CAND [| EXACT_FIRST]
    // LIST: the scan's top-kx list, rows of the caller's batch, LOCAL ids (pads -1)
    const float* list_s = nullptr;
    const int64_t* list_i = nullptr;
    int kx = 0;
    // CAND: a stage's candidate list (workspace rows)
    const key_t64* cand = nullptr;
    unsigned int* cnt = nullptr;
    int cap = 0, dense_n = -1;
    float* thr_s = nullptr;
    key_t64* thr_key = nullptr;
    int kr = 0;                       // slots of the running top-k in the key buffer (power of two >= k)
    int P = 0;                        // key-buffer slots (power of two; LIST: >= kx, CAND: >= 2 * kr)
    // results: rows of the caller's batch
    int k = 0;
    int64_t id_base = 0;
    float* out_scores = nullptr;
    int64_t* out_ids = nullptr;
    float* eps = nullptr;             // [batch rows] the per-query bound (written by LIST)
    unsigned int* flag_word = nullptr;  // LIST: some query is incomplete; CAND: some list lost candidates
    unsigned int* flag_q = nullptr;     // LIST: [batch rows] 0 / 1 per query; CAND: [workspace rows] or NULL
};
// words of an exact-mode store's statistics buffer (device)
constexpr int EXACT_MAX_OUTLIERS = 32;  // per statistic
enum : int { EXS_MAX_N2 = 0, EXS_MAX_D2 = 1, EXS_ORD_N2 = 2, EXS_ORD_D2 = 3, EXS_N_OUT = 4, EXS_CUT_N2 = 5, EXS_CUT_D2 = 6,
             EXS_HIST_N2 = 8, EXS_HIST_D2 = 24, EXS_OUT_ROWS = 64, EXS_WORDS = 64 + 2 * EXACT_MAX_OUTLIERS };
// row_n2 / row_d2: [n_rows] planes of the ingested rows' |x|^2 and |x - x~|^2 (already offset to the first ingested row)
hipError_t launch_ingest_exact(const void* src, int src_dtype, int64_t n_rows, int64_t dim, void* dst16, int dst_dtype, float* dst32,
                               int64_t stride, unsigned int* stats, float* row_n2, float* row_d2, hipStream_t stream);
// re-derive words [EXS_ORD_N2 ..) from the per-row planes of rows [0, n_rows) and the global maxima in words [0], [1]
hipError_t launch_exact_stats(const float* row_n2, const float* row_d2, int64_t n_rows, unsigned int* stats, hipStream_t stream);
hipError_t launch_exact_rescore(const ExactArgs& a, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_listed.hip): scores of listed rows, top-k over a list -------------------
struct ListedArgs {
    const void* plane = nullptr;      // [rows][stride] fp16 / bf16 rows, or the float32 plane of an exact store (`exact`)
    int64_t stride = 0;
    int dim = 0, dim_pad = 0;
    int store_dtype = 0;              // 0 = f16, 1 = bf16: what the query is rounded to (not with `exact`)
    int exact = 0;                    // 1: float32 plane, unrounded query, exact_dot (exact_dot.h)
    const void* q_src = nullptr;      // [nq, dim] of q_dtype
    int q_dtype = 0;
    const int64_t* ids = nullptr;     // [nq, m] listed ids (global: id_base is subtracted)
    int64_t m = 0, id_base = 0, ntotal = 0;
    const int* row_label = nullptr;   // the store's subset labels; read only with q_label
    const int* q_label = nullptr;     // [nq, n_qlab] or NULL = unrestricted
    int n_qlab = 0;
    float* out = nullptr;             // [nq, m]; the weighted sum: [nq, dim]
    int spb = 0;                      // set by the launcher: slots per workgroup, workgroups per query
    int64_t chunks = 0;
    // the weighted sum of listed rows only (q_src / q_dtype are not read there)
    const float* weights = nullptr;   // [nq, m]
    float* part = nullptr;            // temporary: nq * listed_sum_chunks(m) * dim floats; not read when a list is one chunk
};
hipError_t launch_score_listed(ListedArgs a, int64_t nq, hipStream_t stream);
// out[q, :] = sum over the present slots j with weights[q, j] != 0 of weights[q, j] * row(ids[q, j]) (float32 [nq, dim]); one summation
// order per (query, column), fixed by the query's own list and the store's width
int64_t listed_sum_chunks(int64_t m);
hipError_t launch_sum_listed(ListedArgs a, int64_t nq, hipStream_t stream);
// out[q, d] = parts[0][q, d] + parts[1][q, d] + ... in increasing part order; part p of query q starts at parts + p * part_stride + q * q_stride
hipError_t launch_fold_listed_sum(const float* parts, int64_t n_parts, int64_t part_stride, int64_t q_stride, int64_t nq, int dim, float* out,
                                  hipStream_t stream);
// out[i] = parts[owner(ids[i])][i], owner = id / rows_per_shard; -inf where no shard owns the id.  parts: [n_shards][n]
hipError_t launch_combine_listed(const float* parts, const int64_t* ids, int64_t n, int n_shards, int64_t rows_per_shard, float* out,
                                 hipStream_t stream);
// the k best distinct entries of every row of scores / ids [nq, m] (m <= 8192) by (score desc, id asc); NaN and -inf never enter
hipError_t launch_select_listed(const float* scores, const int64_t* ids, int64_t nq, int64_t m, int k, int64_t id_base, float* out_scores,
                                int64_t* out_ids, hipStream_t stream);

// ---- launchers (kernels_l2.hip): the L2 metric around the inner-product scan (VODHIP_L2 stores) ---
// rows: the first of n_rows freshly converted rows [.., stride] (columns >= dim zero); writes the three bias terms of every row
// into columns [dim, dim + 3) and counts rows whose bias saturated into *saturated (l2_bias.h)
hipError_t launch_l2_bias(void* rows, int store_dtype, int64_t n_rows, int64_t dim, int64_t stride, unsigned int* saturated,
                          hipStream_t stream);
// q_src [nq, dim] of q_dtype -> staged [nq, dim + 3] of the store dtype (rounded, saturating; then the three constants), qn [nq] = |q~|^2
hipError_t launch_l2_stage_queries(const void* q_src, int q_dtype, int64_t nq, int64_t dim, int store_dtype, void* staged, float* qn,
                                   hipStream_t stream);
// sim [nq, k] similarity-form scores (pads -inf) -> dist [nq, k] = max(0, qn - 2 sim), pads +inf
hipError_t launch_l2_finish(const float* sim, const float* qn, int64_t nq, int k, float* dist, hipStream_t stream);

// ---- launchers (kernels_update.hip): stored rows changed in place (include/vodhip.h H2u) -----------
enum : int { UPDATE_PLAIN = 0, UPDATE_L2 = 1, UPDATE_EXACT = 2 };  // UpdateArgs::kind
struct UpdateArgs {
    const void* src = nullptr;        // [n_slots, dim] of src_dtype: the source rows of THIS launch's slots
    int src_dtype = 0;
    const int64_t* ids = nullptr;     // device: the id of every slot of the CALL (indexed by the absolute slot), or NULL = the dense form
    int64_t slot_begin = 0;           // this launch's first slot: source row i is slot slot_begin + i
    int64_t n_slots = 0;
    int64_t row_begin = 0;            // dense form: slot j writes row row_begin + j
    int64_t id_base = 0, ntotal = 0;
    int64_t dim = 0, stride = 0;      // stride = the store's dim_pad, of both planes
    int store_dtype = 0;              // 0 = f16, 1 = bf16
    int kind = UPDATE_PLAIN;
    int mode = 0;                     // VODHIP_UPDATE_SET | VODHIP_UPDATE_ADD
    float alpha = 1.f;
    uint16_t* data = nullptr;         // the 16-bit plane
    float* data32 = nullptr;          // UPDATE_EXACT: the float32 plane, the per-row statistics and the two maxima words
    float* row_n2 = nullptr;
    float* row_d2 = nullptr;
    unsigned int* norm_stats = nullptr;
    unsigned int* l2_sat = nullptr;   // UPDATE_L2: the saturation count
    int* owner = nullptr;             // listed form: one word per capacity row, zero between calls
    unsigned int* counts = nullptr;   // listed form: [0] skipped slots, [1] duplicate slots (added to)
};
// listed form, once per call and before its first write launch: owner[row] = 1 + the last slot that lists the row
hipError_t launch_update_claim(const int64_t* ids, int64_t n, int64_t id_base, int64_t ntotal, int* owner, hipStream_t stream);
hipError_t launch_update_rows(const UpdateArgs& a, hipStream_t stream);
// words [EXS_MAX_N2], [EXS_MAX_D2] of an exact store's statistics = the maxima of the finite row_n2 / row_d2 of rows [0, n_rows)
hipError_t launch_update_maxima(const float* row_n2, const float* row_d2, int64_t n_rows, unsigned int* stats, hipStream_t stream);

// ---- launchers (kernels_remove.hip): stored rows removed, the gaps closed in place (include/vodhip.h H2r) -----------
enum : int { RMW_SKIPPED = 0, RMW_DUPLICATES = 1, RMW_FIRST = 2, RMW_WORDS = 4 };  // the call's device words; [RMW_FIRST]: the lowest removed row (starts at ~0u)
struct RemovePlanes {  // one row-indexed set of planes: the store's own, or the bounce buffer's
    uint16_t* data = nullptr;   // [rows][stride]
    float* data32 = nullptr;    // exact store: [rows][stride], and the two statistics per row
    float* row_n2 = nullptr;
    float* row_d2 = nullptr;
    int* label = nullptr;       // row labels, when set
    uint16_t* value = nullptr;  // value table, when attached: [rows][c_pad]
};
struct RemoveGatherArgs {
    RemovePlanes src, dst;            // which planes exist is read from `src`
    const int* owner = nullptr;       // != 0: the row leaves
    const int* tile_off = nullptr;    // exclusive scan of the survivors per count tile
    int64_t tile_base = 0;            // first row of count tile 0 (every row below survives)
    int tile_rows = 256;
    int64_t src_begin = 0, src_rows = 0;  // this launch's source rows
    int64_t dst_sub = 0;              // a survivor with the new id r is written to row r - dst_sub of `dst` (0, or the slab's first new id)
    int64_t stride = 0, c_pad = 0;
    int64_t ntotal = 0;
};
// ids == NULL: the range [row_begin, row_begin + n)
hipError_t launch_remove_mark(const int64_t* ids, int64_t row_begin, int64_t n, int64_t id_base, int64_t ntotal, int* owner, unsigned int* words,
                              hipStream_t stream);
// tile_cnt [n_tiles], tile_off [n_tiles + 1], n_tiles = ceil((ntotal - tile_base) / tile_rows); words[RMW_FIRST] receives the lowest removed row
hipError_t launch_remove_count_scan(const int* owner, int64_t tile_base, int64_t tile_rows, int64_t ntotal, int64_t n_tiles, int* tile_cnt, int* tile_off,
                                    unsigned int* words, hipStream_t stream);
hipError_t launch_remove_gather(const RemoveGatherArgs& a, hipStream_t stream);
hipError_t launch_remove_map(const int* owner, const int* tile_off, int64_t tile_base, int64_t tile_rows, int64_t ntotal, int64_t* new_ids, hipStream_t stream);
}  // namespace vodhip
// what a node index needs of its shards to put them back into the layout `add` fills (vodhip_api.hip; the shards compacted already):
// rows [src_row, src_row + n) of every plane of `src` copied to rows [dst_row, ..) of `dst` on `stream` (an overlapping move inside one
// shard goes through its bounce buffer), and a shard told how many rows it now holds.  Both wait for `stream`.
struct vodhip_index;
namespace vodhip {
int index_remove_move_rows(vodhip_index* src, int64_t src_row, vodhip_index* dst, int64_t dst_row, int64_t n, hipStream_t stream);
int index_remove_set_ntotal(vodhip_index* ix, int64_t ntotal, hipStream_t stream);

// ---- the whole-store scans (store_scan.h): what log_partition, posterior_mean, sample_posterior and the rank calls share ----------
struct ScanInputs {
    const void* store = nullptr;      // [>= round_up(ntotal, 256) rows][dim_pad] fp16 / bf16 rows
    int64_t dim = 0, dim_pad = 0, ntotal = 0;
    int store_dtype = 0;              // 0 = f16, 1 = bf16
    const void* q_src = nullptr;      // the caller's queries [.., dim] of q_dtype
    int q_dtype = 0;
    const int* row_label = nullptr;   // the store's subset labels; read only with q_label
    const int* q_label = nullptr;     // [.., n_qlab] rows of the caller's batch, or NULL = unrestricted
    int n_qlab = 0;
    void* q_stage = nullptr;          // temporary: scan_nq_pad(queries of a launch) * dim_pad 16-bit words
};
int64_t scan_nq_pad(int64_t nq);      // the staged queries of a launch: 64, or a multiple of 128
int64_t scan_tiles(int64_t ntotal);   // 256-row tiles
// queries [q_first, q_first + nq) of the caller's batch -> s.q_stage, rounded to the store dtype and zero padded to [nq_pad][dim_pad]
hipError_t launch_scan_stage(const ScanInputs& s, int64_t q_first, int64_t nq, int64_t nq_pad, hipStream_t stream);
// the subset filter of the slice that starts at query q_first (no q_label: unrestricted)
FilterExtra scan_filter_extra(const ScanInputs& s, int64_t q_first);

// ---- launchers (kernels_partition.hip): log sum exp(beta * score) over the whole store -----------
struct PartitionArgs : ScanInputs {
    float beta = 1.f;
    void* part = nullptr;             // temporary: scan_tiles(ntotal) * scan_nq_pad(nq) float2
    float* out_max = nullptr;         // [rows of the caller's batch]
    float* out_log_rel = nullptr;
};
// queries [q_first, q_first + nq) of the caller's batch -> out_max / out_log_rel [q_first ..); a query's bits do not depend on the split
hipError_t launch_log_partition(const PartitionArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);
// its last launch alone: a.part (written by any scan that restates the partition epilogue) -> out_max / out_log_rel [q_first ..)
hipError_t launch_partition_finish(const PartitionArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_stats.hip): the log-partition pair plus the posterior mean and variance of the score ----
struct StatsArgs : ScanInputs {
    float beta = 1.f;
    void* part = nullptr;             // temporary: scan_tiles(ntotal) * scan_nq_pad(nq) float4
    float* out_max = nullptr;         // [rows of the caller's batch]: the bits of launch_log_partition
    float* out_log_rel = nullptr;
    float* out_mean_rel = nullptr;    // E_p[s] - max
    float* out_var = nullptr;         // Var_p[s]
};
// queries [q_first, q_first + nq) of the caller's batch -> the four outputs [q_first ..); a query's bits do not depend on the split
hipError_t launch_posterior_stats(const StatsArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_divergence.hip): two posteriors over the same rows - each side's (max, log_rel, mean_rel) and the cross moments ----
struct DivergenceArgs : ScanInputs {   // q_src: the queries of side a
    const void* q_src_b = nullptr;    // the queries of side b [.., dim] of q_dtype; q_label: ONE row per pair
    float beta_a = 1.f, beta_b = 1.f;
    void* part = nullptr;             // temporary: scan_tiles(ntotal) * scan_nq_pad(2 nq) float4 (two per (pair, tile))
    float* out[8] = {};               // [pairs of the caller's batch] each: max_a, log_rel_a, mean_rel_a, cross_rel_ab, then side b's
    // q_stage: scan_nq_pad(2 * pairs of a launch) * dim_pad 16-bit words
};
// pairs [q_first, q_first + nq) of the caller's batch -> the eight outputs [q_first ..); a pair's bits do not depend on the split
hipError_t launch_posterior_divergence(const DivergenceArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_rank.hip): exact ranks of listed rows / counts above thresholds over the whole store ----
struct RankArgs : ScanInputs {
    int64_t m = 0, id_base = 0;       // slots per query (1 .. VODHIP_RANK_MAX_LISTED), global id of row 0
    const int64_t* ids = nullptr;     // PICK / RANK: [.., m] listed ids
    const float* thresholds = nullptr;  // THRESHOLDS: [.., m]
    const int64_t* tie_ids = nullptr;   // THRESHOLDS: [.., m], or NULL = strict counts
    // temporaries, sized for P = scan_nq_pad(queries of a launch)
    void* mini = nullptr;             // PICK / RANK: rank_mini_rows(P, m) * dim_pad 16-bit words
    int* slot_row = nullptr;          // PICK / RANK: P * m words
    unsigned int* table = nullptr;    // RANK / THRESHOLDS: 3 * P * m words (keys, tie rows, counts)
    float* out_score = nullptr;       // PICK / RANK: [rows of the caller's batch][m]
    int* out_rows = nullptr;          // PICK / RANK: the same shape, or NULL
    int64_t* out_count = nullptr;     // RANK / THRESHOLDS: the same shape
};
enum : int { RANK_MODE_PICK = 0, RANK_MODE_RANK = 1, RANK_MODE_THRESHOLDS = 2 };
int64_t rank_mini_rows(int64_t nq_pad, int64_t m);
// queries [q_first, q_first + nq) of the caller's batch; a query's results do not depend on the split
hipError_t launch_rank(const RankArgs& a, int mode, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_range.hip): every row above a per-query threshold over the whole store, as a CSR list ----
struct RangeArgs : ScanInputs {
    int64_t id_base = 0;              // global id of row 0
    const float* thresholds = nullptr;  // [rows of the caller's batch]
    const int64_t* tie_ids = nullptr;   // the same shape, or NULL = strict
    // temporaries, sized for P = scan_nq_pad(queries of a launch)
    int* table = nullptr;             // P * scan_tiles(ntotal) words: hits per (query, tile), then their offsets
    unsigned int* words = nullptr;    // 3 * P words: keys, tie rows, hits per query
    unsigned int* status = nullptr;   // RGS_WORDS words, cleared by the caller once per call; NULL without outputs
    int64_t* lims = nullptr;          // [rows of the caller's batch + 1]
    float* out_scores = nullptr;      // [capacity], or NULL: counts and lims only
    int64_t* out_ids = nullptr;
    int64_t capacity = 0;
};
// status words: (query, tile) pairs whose emit count differs from the stored count; emit workgroups that skipped their K loop
enum : int { RGS_SELFCHECK = 0, RGS_SKIPPED = 1, RGS_WORDS = 8 };
// queries [q_first, q_first + nq) of the caller's batch, nq <= 1024; slices run in query order on one stream (lims carries over); a
// query's list does not depend on the split
hipError_t launch_range(const RangeArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_posterior.hip): the posterior mean of the rows, sum_z p(z | q) x_z, behind the log-partition launches ----
struct PosteriorArgs {
    PartitionArgs p;                  // the log-partition call of the same batch: its launches run first, unchanged
    float* acc = nullptr;             // temporary: posterior_mean_groups(ntotal) * scan_nq_pad(nq) * dim_pad floats
    float* out_mean = nullptr;        // [rows of the caller's batch][dim]
};
int64_t posterior_mean_groups(int64_t ntotal);
// queries [q_first, q_first + nq) of the caller's batch -> out_max / out_log_rel (the bits of launch_log_partition) and out_mean rows
// [q_first ..); a query's bits do not depend on the split
hipError_t launch_posterior_mean(const PosteriorArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_readout.hip): the posterior expectation of a per-row value table, sum_z p(z | q) v_z, in ONE scan ----------
struct ReadoutArgs {
    PartitionArgs p;                  // what the log-partition call of the same batch takes: `part` is written by the read-out scan itself
    const void* values = nullptr;     // the table [>= round_up(ntotal, 256) rows][c_pad] of the store dtype, zero padded
    int n_cols = 0, c_pad = 0;        // 1 <= n_cols <= c_pad = 64 * ceil(n_cols / 64) <= 256
    float* acc = nullptr;             // temporary: readout_groups(ntotal) * scan_nq_pad(nq) * c_pad floats
    float* out_values = nullptr;      // [rows of the caller's batch][n_cols]
};
int64_t readout_groups(int64_t ntotal);
// queries [q_first, q_first + nq) of the caller's batch -> out_max / out_log_rel (the bits of launch_log_partition) and out_values rows
// [q_first ..); a query's bits do not depend on the split
hipError_t launch_posterior_expectation(const ReadoutArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_readout_grad.hip): the gradient of that read-out in the query, ONE scan behind the forward's words ---------
struct ReadoutGradArgs {
    PartitionArgs p;                  // the forward's call; out_max / out_log_rel are INPUTS here (the forward's words), `part` is unused
    const void* values = nullptr;     // the table, as ReadoutArgs
    int n_cols = 0, c_pad = 0;
    const float* vmax = nullptr;      // [c_pad] the largest finite |v~| per column (launch_readout_grad_vmax)
    const float* y = nullptr;         // [rows of the caller's batch][n_cols]: the forward's values
    const float* g = nullptr;         // the same shape: dL / dy
    // temporaries, sized for P = scan_nq_pad(queries of a launch)
    void* g_stage = nullptr;          // P * c_pad 16-bit words
    void* aux = nullptr;              // P * readout_grad_aux_bytes()
    float* acc = nullptr;             // readout_groups(ntotal) * P * dim_pad floats
    float* mg = nullptr;              // readout_groups(ntotal) * P floats
    float* out_grad = nullptr;        // [rows of the caller's batch][dim]
};
size_t readout_grad_aux_bytes();
// vmax [c_pad] <- the per-column maxima of the finite |v~| over n_rows rows of the table
hipError_t launch_readout_grad_vmax(const void* values, int64_t n_rows, int c_pad, int store_dtype, float* vmax, hipStream_t stream);
// queries [q_first, q_first + nq) of the caller's batch -> out_grad rows [q_first ..); a query's bits do not depend on the split
hipError_t launch_posterior_expectation_backward(const ReadoutGradArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_readout_adjoint.hip): the read-out's adjoint P^T W, its gradient in the value table; ONE scan, a row per owner ----
struct ReadoutAdjointArgs {
    PartitionArgs p;                  // the forward's call; out_max / out_log_rel are INPUTS here (the forward's words), `part` is unused;
                                      // q_stage: readout_adjoint_nq_pad(queries of a launch) * dim_pad 16-bit words
    const float* w = nullptr;         // [rows of the caller's batch][n_cols]: the weights
    int n_cols = 0, c_pad = 0;        // 1 <= n_cols <= c_pad = 64 * ceil(n_cols / 64) <= 256
    // temporaries
    void* w_stage = nullptr;          // readout_adjoint_nq_pad(queries of a launch) * c_pad 16-bit words
    void* col_k = nullptr;            // c_pad ints: the exponent per weight column (launch_readout_adjoint_columns)
    float* out = nullptr;             // [ntotal][n_cols]
};
int64_t readout_adjoint_nq_pad(int64_t nq);  // the staged queries of a launch: a multiple of 256
// col_k <- the per-column exponents over all nq rows of a.w: once per call, in front of its slices
hipError_t launch_readout_adjoint_columns(const ReadoutAdjointArgs& a, int64_t nq, hipStream_t stream);
// queries [q_first, q_first + nq) of the caller's batch, nq <= 1024 * 1024: out = (add ? out : 0) + their contribution
hipError_t launch_posterior_adjoint(const ReadoutAdjointArgs& a, int64_t q_first, int64_t nq, int add, hipStream_t stream);

// ---- launchers (kernels_key_grad.hip): the posterior's gradient in the stored rows; ONE scan per slice, a row per owner ----
struct KeyGradArgs {
    PartitionArgs p;                  // the forward's call; out_max / out_log_rel are INPUTS here (the forward's words), `part` is unused;
                                      // q_stage: key_grad_nq_pad(queries of a launch) * dim_pad 16-bit words
    const float* a = nullptr;         // [rows of the caller's batch]: dL / d log Z, or NULL = zero
    const float* g = nullptr;         // [rows of the caller's batch][n_cols]: dL / dy, or NULL = zero (no table term is compiled in)
    const float* y = nullptr;         // with g: the forward's values, the same shape
    const void* values = nullptr;     // with g: the table, as ReadoutArgs
    const float* vmax = nullptr;      // with g: [c_pad] the largest finite |v~| per column (launch_readout_grad_vmax)
    int n_cols = 0, c_pad = 0;        // with g: 1 <= n_cols <= c_pad = 64 * ceil(n_cols / 64) <= 256
    // temporaries
    void* g_stage = nullptr;          // with g: key_grad_nq_pad(queries of a launch) * c_pad 16-bit words
    void* aux = nullptr;              // (queries of the CALL) * key_grad_aux_bytes()
    void* scales = nullptr;           // key_grad_scales_bytes(): the batch-wide words (launch_key_grad_scales)
    float* out = nullptr;             // [ntotal][dim]
};
size_t key_grad_aux_bytes();
size_t key_grad_scales_bytes();
int64_t key_grad_nq_pad(int64_t nq);  // the staged queries of a launch: a multiple of 256
// aux, scales <- the per-query words and the batch-wide scales over all nq rows of a.a / a.g / a.y: once per call, in front of its slices
hipError_t launch_key_grad_scales(const KeyGradArgs& a, int64_t nq, hipStream_t stream);
// queries [q_first, q_first + nq) of the caller's batch, nq <= 1024 * 1024: out = (add ? out : 0) + their contribution
hipError_t launch_posterior_key_gradient(const KeyGradArgs& a, int64_t q_first, int64_t nq, int add, hipStream_t stream);

}  // namespace vodhip
struct vodhip_index;
namespace vodhip {
// the key gradient of one shard of a node index (vodhip_api.hip).  index_value_vmax: the shard's cached column maxima of its part of
// the value table [c_pad] to the host (computed on first use; waits for `stream`).  index_posterior_key_gradient: the flat call with
// the column maxima the batch-wide scales are formed from handed in (DEVICE [c_pad]; NULL without grad_values), no accumulate
int index_value_vmax(vodhip_index* ix, float* vmax_host, int64_t c_pad, hipStream_t stream);
int index_posterior_key_gradient(vodhip_index* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev, int n_per_query,
                                 const float* max_score, const float* log_rel, const float* grad_log_z, const float* values, const float* grad_values,
                                 const float* vmax_dev, float* out, hipStream_t stream);

// ---- launchers (kernels_sample_posterior.hip): k rows without replacement from p(z | q) over the whole store --------------------
struct PosteriorSampleArgs {
    PartitionArgs p;                  // the log-partition call of the same batch: its launches run first, unchanged
    int k = 0;                        // 1 .. 255
    uint64_t seed = 0;
    int64_t query_offset = 0;         // stream index of query 0 of the caller's batch
    int64_t id_base = 0;              // global id of row 0
    int64_t stride = 0;               // candidate slots per query: sample_posterior_stride(ntotal, k)
    // temporaries, sized for P = scan_nq_pad(queries of a launch)
    float* keymax = nullptr;          // P * scan_tiles(ntotal) floats
    void* cand_key = nullptr;         // P * stride 64-bit keys
    float* cand_score = nullptr;      // P * stride floats
    unsigned int* ctl = nullptr;      // sample_posterior_ctl_words(P) words: counters, hit tiles, thresholds (cleared by every launch)
    unsigned int* status = nullptr;   // 8 words, cleared by the caller once per call: [0] queries whose list overflowed, [1] queries with
                                      // fewer candidates than hit tiles, [2] largest list, [3] emit workgroups that skipped their K loop,
                                      // [4..5] candidates in all (64 bits)
    int64_t* out_ids = nullptr;       // [rows of the caller's batch][k]
    float* out_scores = nullptr;
    float* out_log_p = nullptr;
    float* out_log_weight = nullptr;
    float* out_keys = nullptr;        // [..][k + 1]
    hipEvent_t* ev = nullptr;         // NULL, or 6 events: [1] .. [5] are recorded behind the log-partition launches, the key-max scan,
                                      // the threshold, the emit scan and the select ([0] is the caller's, in front)
};
int64_t sample_posterior_stride(int64_t ntotal, int k);
int64_t sample_posterior_ctl_words(int64_t nq_pad);
// queries [q_first, q_first + nq) of the caller's batch; a query's bits do not depend on the split
hipError_t launch_sample_posterior(const PosteriorSampleArgs& a, int64_t q_first, int64_t nq, hipStream_t stream);

// ---- launchers (kernels_hybrid.hip) -----------------------------------------------------------
struct HybridArgs {
    const int64_t* lookup_idx;
    const int64_t* lookup_lbl;
    int k_lookup;
    int n_engines;
    const int64_t* engine_idx[4];
    const float* engine_scr[4];
    int engine_k[4];
    float engine_w[4];
    int64_t nq;
    int64_t* out_idx;
    float* out_scr;
    int64_t* out_lbl;
    float* out_raw[4];
    int out_stride;
    int32_t* out_width;        // [4] maximum over rows of the cursor after each engine (atomics; cleared by the launcher), or NULL
    int32_t* out_row_cursor;   // [nq, 4] the same cursors per row (plain stores), or NULL
};
hipError_t launch_merge_hybrid(const HybridArgs& a, hipStream_t stream);

// ---- launchers (kernels_retrieval.hip) --------------------------------------------------------
// auxiliary losses of the retrieval objective (passed by value; `enabled` = 0 leaves the plain loss and an 8-float row stride)
struct RetrievalAux {
    int enabled = 0;
    int guidance_type = 0;   // 0 = "zero", 1 = "sparse"
    float w_guidance = 0.f, w_self = 0.f, w_decay = 0.f;
    float* grad = nullptr;   // [3][B*D] scratch: unnormalised gradients of the three terms w.r.t. the scores
    float* out = nullptr;    // [3] loss values: guidance, self-supervision, score decay (NaN where the weight is 0)
};
hipError_t launch_retrieval_forward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D,
                                    int64_t H, const float* score, const int64_t* relevance, const float* sparse,
                                    const float* dense, float* retriever_scores, float* d_scores, float* loss,
                                    float* kl, float* workspace, const RetrievalAux& aux, hipStream_t stream,
                                    int64_t workspace_floats = 0);
hipError_t launch_retrieval_backward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D,
                                     int64_t H, const float* d_scores, const float* grad_out, float* dq, float* ds,
                                     hipStream_t stream);
// C[M,N] (f32) = *alpha (device scalar, or NULL = 1) * A[M,K] * B[K,N] on the exact-f32 MFMA; element strides; dtype pairs (dta, dtb):
// (0,0) (1,1) (2,2) (2,0) (2,1).  n_splits > 1: K split over blockIdx.z, split z writes the slab C + z * c_split_stride (the consumer
// sums the slabs in order).
hipError_t launch_small_gemm(int dta, int dtb, const void* A, int64_t sa_m, int64_t sa_k, const void* B, int64_t sb_k,
                             int64_t sb_n, float* C, int64_t ldc, int M, int N, int K, const float* alpha,
                             hipStream_t stream, int n_splits = 1, int64_t c_split_stride = 0);

// ---- launchers (kernels_pool.hip) -------------------------------------------------------------
struct PoolPlan {
    int64_t l_chunk;   // tokens per workgroup
    int64_t n_chunks;  // workgroups per row; 1 = the single-launch path, no workspace
};
PoolPlan pool_plan(int64_t N, int64_t L, int64_t H, int64_t l_chunk);  // l_chunk = 0: automatic, from (N, L, H) alone
hipError_t launch_pool_forward(const void* hidden, int dtype, int64_t N, int64_t L, int64_t H, const void* mask, int mask_eb, int agg,
                               int masked, int finish, int act, int norm, const float* log_scaler, int64_t l_chunk, float* a, void* y,
                               int y_dtype, float* workspace, hipStream_t stream);
hipError_t launch_pool_backward(const void* g, int g_dtype, const float* a, int64_t N, int64_t L, int64_t H, const void* mask,
                                int mask_eb, int agg, int masked, int finish, int act, int norm, const float* log_scaler,
                                int64_t l_chunk, void* d_hidden, int dtype, float* gy, hipStream_t stream);
hipError_t launch_pool_finish_forward(const void* z, int z_dtype, int64_t N, int64_t P, int act, int norm, const float* log_scaler,
                                      void* y, int y_dtype, hipStream_t stream);
hipError_t launch_pool_finish_backward(const void* z, int z_dtype, const void* g, int g_dtype, int64_t N, int64_t P, int act, int norm,
                                       const float* log_scaler, void* dz, int dz_dtype, float* gy, hipStream_t stream);

// ---- launchers (kernels_marginal.hip) ---------------------------------------------------------
// mask_eb: bytes per attention-mask element (1 | 2 | 4 | 8; an element is live when any of its bits is set)
hipError_t launch_lm_token_forward(const void* logits, int dtype, int64_t N, int64_t L, int64_t V, const int64_t* ids,
                                   const void* mask, int mask_eb, float* tok_logp, float* tok_lse, hipStream_t stream);
hipError_t launch_lm_token_backward(const void* logits, int dtype, int64_t N, int64_t L, int64_t V, const int64_t* ids,
                                    const void* mask, int mask_eb, const float* tok_lse, const float* coef, const float* grad_out,
                                    void* d_logits, hipStream_t stream);
hipError_t launch_marginal_forward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                                   const float* score, const float* tok_logp, const void* mask, int mask_eb, int64_t L,
                                   float* retriever_scores, float* d_scores, float* coef, float* loss, float* workspace,
                                   int64_t workspace_floats, hipStream_t stream);
// eps = 1 - alpha; log_proposal may be NULL (temperature * score); tok_mean: 1 = mean over the live tokens, 0 = their sum
hipError_t launch_vod_forward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                              const float* score, const float* log_weight, const float* log_proposal, const float* tok_logp,
                              const void* mask, int mask_eb, int64_t L, float eps, float temperature, int tok_mean,
                              float* retriever_scores, float* d_scores, float* coef, float* loss, float* diag, float* workspace,
                              int64_t workspace_floats, hipStream_t stream);

// ---- launchers (kernels_sample.hip) -----------------------------------------------------------
hipError_t launch_priority_sample(const float* scores, const uint8_t* labels, const float* noise, int64_t nq, int width,
                                  int k_positive, int k_total, float temperature, int max_support_size, int normalized,
                                  int64_t* out_samples, float* out_log_weights, uint8_t* out_labels, float* out_lse,
                                  float* out_log_proposal, float* out_log_mass, float* out_joint_logw, hipStream_t stream);

// sampling straight from the merge's full-stride outputs + the gather epilogue (device-resident collate)
struct SampleMergedArgs {
    const int64_t* ids;
    const float* scores;
    const int64_t* labels;   // > 0 = positive
    const float* noise;
    int64_t nq, stride, noise_stride;
    int width;               // >= 0: columns in use; < 0: derived on the device from merge_width / k_lookup / engine_k
    const int* merge_width;  // [n_engines] maxima over rows, or NULL
    const int* row_cursor;   // [nq, 4] per-row cursors (the kernel takes the maximum), or NULL
    int k_lookup, n_engines, engine_k[4];
    int k_positive, k_total;
    float temperature;
    int max_support, normalized;
    int n_raw;
    const float* raw[4];
    int64_t* out_samples;
    int64_t* out_ids;
    float* out_scores;
    float* out_logw;
    uint8_t* out_labels;
    float* out_raw[4];
    float* out_lse;          // lse of class c of row r at out_lse[r * lse_row_stride + c * lse_cls_stride]
    int64_t lse_row_stride, lse_cls_stride;
    float* out_max_sampling_id;
    // the sampler's proposal, each NULL or: log_p of the samples [nq, k_total]; log_mass of class c of row r at
    // out_log_mass[r * lse_row_stride + c * mass_cls_stride]; joint log-weights [nq, k_total] (needs bit 0 of `normalized`)
    float* out_log_proposal;
    float* out_log_mass;
    int64_t mass_cls_stride;
    float* out_joint_logw;
};
hipError_t launch_priority_sample_merged(const SampleMergedArgs& m, hipStream_t stream);
hipError_t launch_flatten_inbatch(const int64_t* ids, int64_t n_rows, int n_keys, int n_values, const float* const* values,
                                  const float* fill, float* const* outs, const uint8_t* labels, uint8_t* out_labels,
                                  int64_t* out_unique, int* out_n_unique, hipStream_t stream);

hipError_t launch_gather_by_id(const int64_t* queries, int64_t n_queries, const int64_t* keys, int64_t n_rows, int n_keys,
                               int n_values, const float* const* values, const float* fill, float* const* outs,
                               hipStream_t stream);

// ---- launchers (kernels_metrics.hip) ----------------------------------------------------------
// the (metric, topk) list of one monitor update, passed to the kernel by value
struct MetricSpecs {
    int n;
    int metric[32];  // VODHIP_METRIC_*
    int topk[32];    // 0 = no cut
};
// per-row values -> values [specs.n][B] (required); state [specs.n][2] += (sum, count of the non-NaN values) when not NULL
hipError_t launch_retrieval_metrics(const float* scores, const int64_t* relevances, int64_t B, int width, const MetricSpecs& specs,
                                    float* values, double* state, hipStream_t stream);

}  // namespace vodhip
