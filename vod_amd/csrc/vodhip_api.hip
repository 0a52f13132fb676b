// C-ABI layer of libvodhip.so: handle management, ingest, the chunk schedule of the fused
// score + top-k search, and thin wrappers for the merge / hybrid / retrieval kernels.
// See include/vodhip.h for the contract and the reference call sites each entry point replaces.
#include "../../include/vodhip.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <deque>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <vector>

#include "l2_bias.h"
#include "partition_fold.h"
#include "sample_fold.h"
#include "rank_fold.h"
#include "range_fold.h"
#include "stats_fold.h"
#include "divergence_fold.h"
#include "readout_fold.h"
#include "readout_adjoint_fold.h"
#include "readout_grad_fold.h"
#include "key_grad_fold.h"
#include "update_fold.h"
#include "remove_fold.h"
#include "scan_slices.h"
#include "search_plan.h"
#include "collate_plan.h"
#include "vodhip_internal.h"

using namespace vodhip;

namespace {

thread_local std::string g_last_error;

int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return -1;
}

}  // namespace

namespace vodhip {
void set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }
}  // namespace vodhip

namespace {

#define HIP_OK(expr)                                                                            \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            (void)hipGetLastError(); /* reported here: must not resurface in a later launch check */ \
            return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                       \
    } while (0)

constexpr int64_t STAGE_BYTES = 64ll << 20;

struct PendingSearch {
    bool active = false;
    const void* queries = nullptr;
    int q_dtype = 0;
    int64_t nq = 0;
    int k = 0;
    int64_t id_base = 0;
    float* out_scores = nullptr;
    int64_t* out_ids = nullptr;
    const int* q_label = nullptr;  // subset labels in force when the search was enqueued
    int n_qlab = 0;
    const int* q_map = nullptr;    // recovery of a few queries: workspace row -> row of the caller's batch (device)
    int slot = 0;                  // overflow-flag word / completion event of this search
    size_t ev_begin = 0, ev_end = 0;  // profile events of this search in ev_pool
    int kx = 0;                    // exact mode: the scan's list length k' (> k; 0 = not an exact-mode search)
    bool band = false;             // exact mode: a BAND pass - candidates are re-scored into the caller's rows (kernels_exact.hip)
    bool defer_flags = false;      // exact mode: the flag words are fetched (and the slot's event recorded) behind the re-scoring launch
    int lane = 0;                  // which of the index's two workspaces / streams this search runs on (1 = the index's own stream)
    float* l2_out = nullptr;       // L2 store: the caller's out_scores (out_scores above is the slot's similarity-form buffer, queries its staged copy)
};

constexpr int FLAG_WORDS = 4;     // flag words of a workspace / of a slot's host copy ([3]: blocks that missed the survivor rings)
constexpr int MAX_IN_FLIGHT = 4;  // searches that may be enqueued before the oldest is finished
constexpr int64_t OVF_ROWS = 65536;  // per-query overflow flags are kept for batches up to this many queries

}  // namespace

struct vodhip_index {
    int device = 0;
    int64_t dim = 0, dim_pad = 0;
    int64_t dim_s = 0;               // columns a search contracts over: dim, or dim + 3 for an L2 store (the bias columns, l2_bias.h)
    int64_t capacity = 0, capacity_pad = 0;
    int64_t ntotal = 0;
    int dtype = VODHIP_F16;
    uint16_t* data = nullptr;
    int* row_label = nullptr;        // [capacity_pad] subset label per row (optional)
    // the value table of the posterior read-out (kernels_readout.hip): [round_up(value_rows, 256)][value_c_pad] of the store dtype, zero padded
    uint16_t* row_value = nullptr;
    int64_t value_rows = 0, value_cols = 0, value_c_pad = 0;
    int64_t value_alloc_rows = 0;    // rows the table was allocated for (>= round_up(value_rows, 256): vodhip_index_remove_rows shrinks value_rows)
    // beside it: the per-column maxima of the finite |v~| (kernels_readout_grad.hip), computed by the first backward call after the
    // table was set (under `mu`) and dropped with the table
    float* value_vmax = nullptr;     // [value_c_pad]
    bool value_vmax_ready = false;
    const int* q_label = nullptr;    // caller-owned device [nq, n_qlab] for the next searches (optional)
    int n_qlab = 0;
    // host ingest pipeline: two slots of (pinned host staging, device staging of the raw dtype, completion event), one stream
    void* stage_dev[2] = {nullptr, nullptr};
    void* stage_pin[2] = {nullptr, nullptr};
    hipEvent_t stage_done[2] = {nullptr, nullptr};
    int64_t ingest_threads = 0;  // CPU threads that fill the pinned staging slots (0 = auto: min(8, hardware threads))
    int64_t last_ingest_pinned_src = 0;
    // vodhip_index_update_rows, listed form (kernels_update.hip): the owner word per capacity row (zero between calls), the call's
    // (skipped, duplicates) words, the ids of a host call; allocated by the first listed call.  last_update_n / _listed: the slots of
    // the last call and whether it had a list (a dense call writes them all and has nothing to read back)
    int* upd_owner = nullptr;
    unsigned int* upd_counts = nullptr;
    int64_t* upd_ids = nullptr;
    int64_t upd_ids_cap = 0;
    int64_t last_update_n = 0;
    bool last_update_listed = false;
    // vodhip_index_remove_rows (kernels_remove.hip; it shares upd_owner / upd_ids): the call's device words, the survivor counts per
    // count tile and their scan, and the BOUNCE buffer - one slab of every plane the store keeps, min(remove_slab_rows, capacity) rows
    // of 2 * dim_pad bytes (+ 4 * dim_pad + 8 of an exact store, + 4 with labels, + 2 * value_c_pad with a table): 100 MB for 65536
    // fp16 rows of 768 columns, 300 MB for an exact store.  Allocated by the first call that needs them, grown when a plane was added
    unsigned int* rm_words = nullptr;
    int* rm_tiles = nullptr;          // [2 * rm_tiles_cap + 1]: counts, then offsets
    int64_t rm_tiles_cap = 0;
    char* rm_bounce = nullptr;
    size_t rm_bounce_bytes = 0;
    int64_t remove_slab_rows = REMOVE_SLAB_ROWS;
    int64_t last_remove[3] = {0, 0, 0};  // removed, skipped, duplicates of the last call
    // VODHIP_EXACT_F32 (kernels_exact.hip): the float32 rows, the statistics of the error bound, per-slot lists of the scan
    bool exact = false;
    float* data32 = nullptr;                 // [capacity + 1][dim_pad]
    unsigned int* norm_stats = nullptr;      // device [EXS_WORDS]: max |x|^2, max |x - x~|^2 (atomics at ingest), the ordinary maxima, the outliers
    float* row_n2 = nullptr;                 // device [capacity + 1]: |x|^2 of every row (written at ingest)
    float* row_d2 = nullptr;                 // device [capacity + 1]: |x - x~|^2
    bool stats_dirty = true;                 // rows were added / updated / the store was reset since the statistics below were derived
    bool maxima_stale = false;               // rows were updated since the two maxima words were derived: they may belong to rows that left
    float ord_n2 = 0.f, ord_d2 = 0.f, cut_n2 = 0.f, cut_d2 = 0.f;  // host copies (refresh_exact_stats): the bound's maxima over the ordinary rows, the outlier cuts
    int n_out = 0;                           // outlier rows (scored by every query instead of bounded)
    int64_t exact_adapt = 1;                 // 1: the list length k' follows what the last searches needed (0: always the formula)
    int adapt_k = 0, adapt_kx = 0;           // the k the adapted k' belongs to / the adapted k' (0 = none yet)
    int64_t last_exact_need = 0;             // list entries within eps of the k-th exact score, maximum over the last search's queries
    float* x_list_s[4] = {nullptr, nullptr, nullptr, nullptr};     // per in-flight slot: the scan's top-k' list [nq][k']
    int64_t* x_list_i[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t x_list_cap[4] = {0, 0, 0, 0};     // elements
    float* x_eps = nullptr;                  // device [MAX_IN_FLIGHT][OVF_ROWS]: the per-query bound of a slot's search
    unsigned int* x_flag_q = nullptr;        // device [MAX_IN_FLIGHT][OVF_ROWS]: the queries whose list did not prove complete
    int64_t exact_expand_x100 = 0;           // k' = k * this / 100 (+ 16); 0 = by store dtype (fp16: 110, bf16: 200)
    int64_t last_exact_kx = 0, last_exact_band_queries = 0, last_exact_band_passes = 0;
    // VODHIP_L2 (kernels_l2.hip): rows carry three bias columns behind the user's dim; per in-flight slot the staged queries
    // [nq][dim + 3], their squared norms and the search's similarity-form scores [nq][k] (the recovery passes seed from them)
    bool l2 = false;
    unsigned int* l2_sat = nullptr;          // device word: rows whose bias saturated since create / reset
    uint16_t* l2_q[4] = {nullptr, nullptr, nullptr, nullptr};
    float* l2_qn[4] = {nullptr, nullptr, nullptr, nullptr};
    float* l2_sim[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t l2_q_cap[4] = {0, 0, 0, 0}, l2_qn_cap[4] = {0, 0, 0, 0}, l2_sim_cap[4] = {0, 0, 0, 0};  // elements
    hipEvent_t l2_ev[4][4] = {};             // with "profile": per slot, (start, stop) around the staging and around the finish launch
    int64_t last_l2_stage_ns = 0, last_l2_finish_ns = 0;
    // Two LANES: workspace 0 is used on the caller's stream; workspace 1 on a stream of the index's own, so that two consecutive searches
    // of a caller that runs one search ahead (the bench, the batcher) overlap on the device: while one search's select / prepare launches
    // and the partly filled last round of its stage leave CUs idle, the other search's FILTER workgroups take them.  Used for batches of
    // one query tile (param "lanes": 0 = auto, 1, 2), where those gaps are ~12 % of a 1 M-row search (profiles/r05_ab_lanes.txt).
    SearchWorkspace ws_lane[2];
    hipStream_t lane_stream = nullptr;
    hipEvent_t lane_in[4] = {};              // recorded on the caller's stream at enqueue: lane 1 starts behind the caller's pending work
    int64_t lanes = 0;
    unsigned int* overflow_host = nullptr;  // pinned, FLAG_WORDS per in-flight slot: [0] a candidate list overflowed, [1] exact mode: some list did not prove complete, [2] exact mode: max over queries of the list entries within eps of the k-th exact score
    unsigned int* ovf_q = nullptr;          // device [MAX_IN_FLIGHT][OVF_ROWS]: which queries of a slot's search overflowed
    int* q_map = nullptr;                   // device [MAX_IN_FLIGHT][OVF_ROWS]: the rows a slot's recovery pass re-searches
    hipEvent_t done[MAX_IN_FLIGHT] = {};    // recorded after a search's overflow word is copied back
    std::deque<PendingSearch> inflight;     // oldest first
    int unfinished = 0;                     // searches popped by a vodhip_index_search_finish that is still waiting for their event
    int next_slot = 0;
    // tunables
    PlanTunables tune;  // the planner's (n_cu: read once at create)
    int64_t force_safe = 0;
    int64_t kflags = 0;
    int64_t profile = 0;  // 1: bracket every filter launch with HIP events (bench / roofline accounting)
    int64_t scan_temp_bytes = VODHIP_POSTERIOR_TEMP_BYTES;  // what the sliced whole-store scans keep their temporaries under (scan_slices.h)
    // stats
    int64_t last_overflow = 0, last_chunks = 0, last_survivor_ring = 0, last_ring_fallbacks = 0, last_safe_reruns = 0, last_recovered_queries = 0;
    int64_t last_filter_launches = 0, last_filter_ns = 0;
    int64_t last_recovery_launches = 0, last_recovery_ns = 0;  // filter launches of the recovery passes (with "profile")
    // the last vodhip_index_sample_posterior: its status words, the emit launches' workgroups, with "profile" the ns per launch
    std::atomic<int64_t> last_sample[6] = {};      // overflow, selfcheck, max candidates, emit skipped, candidates, emit groups
    std::atomic<int64_t> last_sample_ns[5] = {};   // partition, keymax, threshold, emit, select
    std::atomic<int64_t> last_scan[2] = {};        // the last sliced whole-store scan: queries (or pairs) per slice, temporary bytes per query
    std::atomic<int64_t> last_range[4] = {};       // the last vodhip_index_range_search: overflow, selfcheck, emit skipped, emit groups
    // its temporaries: one grow-only block, kept between calls (the call waits for its stream at its end, and a stream-ordered pool
    // hands its memory back at every such wait: allocating per call cost 1.1 ms of a 3.8 ms call at 256 queries); held by
    // sample_mu for the length of a call, so two calls on one index run one after the other
    void* sample_ws = nullptr;
    size_t sample_ws_bytes = 0;
    std::mutex sample_mu;
    std::vector<hipEvent_t> ev_pool;  // pairs (start, stop), reused across searches
    size_t ev_used = 0;
    // Every entry point that touches `inflight`, the shared workspace (`ws`, incl. its host-side `extra`) or the event pool holds
    // this: a server thread may enqueue search i + 1 while another completes (and, after an overflow, RE-ENQUEUES recovery passes of)
    // search i on the same handle.  The wait for a search's completion event happens outside it.
    std::mutex mu;
};

namespace {

int elem_size(int dtype) { return dtype == VODHIP_F32 ? 4 : 2; }

int free_workspace(vodhip_index* ix, int lane) {
    SearchWorkspace& w = ix->ws_lane[lane];
    (void)hipFree(w.q_pad);
    (void)hipFree(w.topk);
    (void)hipFree(w.cand);
    (void)hipFree(w.cnt);
    (void)hipFree(w.thr_s);
    (void)hipFree(w.thr_key);
    (void)hipFree(w.overflow);
    (void)hipFree(w.ring);
    const int n_cu = w.n_cu;
    w = SearchWorkspace();
    w.n_cu = n_cu;
    return 0;
}

int ensure_workspace(vodhip_index* ix, int lane, int64_t nq_pad, int64_t cap, int64_t kp) {
    SearchWorkspace& w = ix->ws_lane[lane];
    // (kp: the running top-k's row stride of THIS search, passed to the launches by value; the buffer is sized for the widest seen - an
    // exact-mode scan (k') and its band pass (k) alternate between two widths: reallocating per search is a device-wide hipFree each time)
    if (w.nq_cap >= nq_pad && w.cap == cap && w.kp_cap >= kp && w.q_pad) {
        w.kp = kp;
        return 0;
    }
    const int64_t nq_cap = std::max(nq_pad, w.nq_cap);
    const int64_t kp_cap = std::max(kp, w.kp_cap);
    free_workspace(ix, lane);
    HIP_OK(hipMalloc((void**)&w.q_pad, (size_t)nq_cap * ix->dim_pad * 2));
    HIP_OK(hipMalloc((void**)&w.topk, (size_t)nq_cap * kp_cap * sizeof(key_t64)));
    HIP_OK(hipMalloc((void**)&w.cand, (size_t)nq_cap * cap * sizeof(key_t64)));
    HIP_OK(hipMalloc((void**)&w.cnt, (size_t)nq_cap * CNT_STRIDE * sizeof(unsigned int)));
    HIP_OK(hipMalloc((void**)&w.thr_s, (size_t)nq_cap * sizeof(float)));
    HIP_OK(hipMalloc((void**)&w.thr_key, (size_t)nq_cap * sizeof(key_t64)));
    HIP_OK(hipMalloc((void**)&w.overflow, FLAG_WORDS * sizeof(unsigned int)));  // [0] overflow, [1] exact mode's "incomplete" word, [2] its "needed list length"
    w.nq_cap = nq_cap;
    w.cap = cap;
    w.kp = kp;
    w.kp_cap = kp_cap;
    return 0;
}

// the survivor rings of the 8-phase kernel for `records` per wave (SearchPlan::ring), on the largest grid its launcher makes: one workgroup
// per CU, at least 8 per query tile (<= 64: MAX_NQ_PER_PASS / 256 query tiles).  The rings only buy speed: when the device cannot hold
// them the search runs without (ring_cap 0: every block takes the in-loop path), it does not fail.
int ensure_ring(vodhip_index* ix, int lane, int64_t records) {
    SearchWorkspace& w = ix->ws_lane[lane];
    const int64_t floats = (int64_t)std::max(w.n_cu, 64) * 8 * records * 33;
    if (floats > w.ring_floats) {
        (void)hipFree(w.ring);
        w.ring = nullptr;
        w.ring_floats = 0;
        if (hipMalloc((void**)&w.ring, (size_t)floats * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();  // (not sticky for the launches that follow)
            w.ring = nullptr;
            w.ring_cap = 0;
            return 0;
        }
        w.ring_floats = floats;
    }
    w.ring_cap = records;
    return 0;
}

// exact mode: the statistics of the error bound as the re-scoring launches take them (host copies: refresh_exact_stats)
void exact_bound_args(const vodhip_index* ix, ExactArgs& xa) {
    xa.ord_n2 = ix->ord_n2;
    xa.ord_d2 = ix->ord_d2;
    xa.cut_n2 = ix->cut_n2;
    xa.cut_d2 = ix->cut_d2;
    xa.n_out = ix->n_out;
    xa.out_rows = ix->norm_stats + EXS_OUT_ROWS;
    xa.row_n2 = ix->row_n2;
    xa.row_d2 = ix->row_d2;
}

// exact mode, before the first search after rows were added (no search is in flight then: `add` refuses otherwise): re-derive the maxima
// of the bound over the ORDINARY rows and the list of outliers from the per-row planes (8 bytes per row: ~30 us for 10 M rows), and
// fetch them.  ONE host sync per batch of adds.
int refresh_exact_stats(vodhip_index* ix, hipStream_t stream) {
    if (!ix->exact || !ix->stats_dirty) return 0;
    // rows were updated in place: the maxima the ingest launches kept may belong to rows that left.  They do not make a result wrong,
    // but they place the outlier cuts (level_of: M / 4^j) - re-derive them from the rows now stored (8 bytes per row)
    if (ix->maxima_stale) HIP_OK(launch_update_maxima(ix->row_n2, ix->row_d2, ix->ntotal, ix->norm_stats, stream));
    ix->maxima_stale = false;
    HIP_OK(launch_exact_stats(ix->row_n2, ix->row_d2, ix->ntotal, ix->norm_stats, stream));
    unsigned int w[8];
    HIP_OK(hipMemcpyAsync(w, ix->norm_stats, sizeof(w), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    auto f = [](unsigned int u) { float v; memcpy(&v, &u, 4); return v; };
    ix->ord_n2 = f(w[EXS_ORD_N2]);
    ix->ord_d2 = f(w[EXS_ORD_D2]);
    ix->cut_n2 = f(w[EXS_CUT_N2]);
    ix->cut_d2 = f(w[EXS_CUT_D2]);
    ix->n_out = (int)std::min<unsigned int>(w[EXS_N_OUT], 2u * EXACT_MAX_OUTLIERS);
    if (w[EXS_N_OUT] > 2u * EXACT_MAX_OUTLIERS) return fail("internal error: %u outlier rows", w[EXS_N_OUT]);
    ix->stats_dirty = false;
    return 0;
}

// one stage's filter launch on a pass of nq queries, bracketed by profile events (bench / roofline accounting)
int launch_stage(vodhip_index* ix, SearchWorkspace& W, const SearchPlan& plan, const Stage& sg, int64_t nq, int64_t nq_pad,
                 FilterStageFn experiment, hipStream_t stream) {
    hipEvent_t ev1 = nullptr;
    if (ix->profile) {
        while (ix->ev_pool.size() < ix->ev_used + 2) {
            hipEvent_t ev;
            HIP_OK(hipEventCreate(&ev));
            ix->ev_pool.push_back(ev);
        }
        hipEvent_t ev0 = ix->ev_pool[ix->ev_used++];
        ev1 = ix->ev_pool[ix->ev_used++];
        HIP_OK(hipEventRecord(ev0, stream));
    }
    W.extra.sample_rstride = (int)sg.rstride;
    W.extra.sample_offset = (int)sg.sample_offset;
    W.extra.sample_groups = (int)sg.n_groups;
    HIP_OK(launch_filter(ix->dtype, plan.kernel(sg, nq_pad), sg.kind, ix->data, W.q_pad, ix->dim_pad, sg.b, sg.e, sg.n_tiles, nq, nq_pad, W,
                         stream, experiment));
    if (ix->profile) HIP_OK(hipEventRecord(ev1, stream));
    return 0;
}

// exact mode (a BAND pass): the re-scoring of stage `sg`'s candidates from the float32 plane into the caller's rows [row0, row0 + nq)
ExactArgs exact_stage_args(const vodhip_index* ix, const PendingSearch& ps, const SearchWorkspace& ws, int64_t row0, const Stage& sg, bool first) {
    ExactArgs xa;
    xa.plane = ix->data32;
    xa.stride = ix->dim_pad;
    xa.dim = (int)ix->dim;
    xa.dim_pad = (int)ix->dim_pad;
    xa.q_src = (const char*)ps.queries + (size_t)row0 * ix->dim * elem_size(ps.q_dtype);
    xa.q_dtype = ps.q_dtype;
    xa.q_map = ws.extra.q_map;
    xa.store_dtype = ix->dtype;
    exact_bound_args(ix, xa);
    xa.row_label = ws.extra.row_label;
    xa.q_label = ws.extra.q_label;
    xa.n_qlab = ws.extra.n_qlab;
    xa.mode = EXACT_CAND | (first ? EXACT_FIRST : 0);
    xa.cand = ws.cand;
    xa.cnt = ws.cnt;
    xa.cap = (int)ws.cap;
    xa.dense_n = sg.kind == ST_DENSE ? (int)(sg.e - sg.b) : -1;
    xa.thr_s = ws.thr_s;
    xa.thr_key = ws.thr_key;
    xa.kr = 2;
    while (xa.kr < ps.k) xa.kr <<= 1;
    xa.P = std::max(2 * xa.kr, 1024);
    xa.k = ps.k;
    xa.id_base = ps.id_base;
    xa.out_scores = ps.out_scores + row0 * ps.k;
    xa.out_ids = ps.out_ids + row0 * ps.k;
    xa.flag_word = ws.overflow;
    return xa;
}

int enqueue_search_impl(vodhip_index* ix, const PendingSearch& ps, bool safe, int recovery, hipStream_t stream) {
    SearchWorkspace& W = ix->ws_lane[ps.lane];  // this search's lane
    const int k = ps.k;
    int64_t kp = 64;
    while (kp < k) kp <<= 1;
    const int64_t cap = ix->tune.cand_cap;
    if (cap / ROW_ALIGN * ROW_ALIGN < k) return fail("cand_cap=%lld is too small for k=%d", (long long)cap, k);

    // the subset labels in force when THIS search was enqueued (a recovery pass may run after younger searches changed them)
    const int* row_label = (ix->row_label && ps.q_label) ? ix->row_label : nullptr;
    PlanTunables tune = ix->tune;
    const FilterStageFn experiment = experiment_filter(tune);
    const SearchPlan plan = plan_search(ix->ntotal, k, ps.nq, tune, row_label != nullptr, safe, recovery);
    ix->last_chunks = (int64_t)plan.stages.size();
    ix->last_survivor_ring = plan.ring;

    const int q_es = elem_size(ps.q_dtype);
    if (ensure_workspace(ix, ps.lane, round_up(std::min(MAX_NQ_PER_PASS, ps.nq), 256), cap, kp)) return -1;
    if (ensure_ring(ix, ps.lane, plan.ring)) return -1;
    W.extra.flags = ((int)ix->kflags << 8) | (plan.corpus_nt ? FILTER_FLAG_CORPUS_NT : 0);  // (the knobs: diagnostic builds only)
    W.extra.row_label = row_label;
    W.extra.n_qlab = ps.n_qlab;
    W.extra.perm_mul = (int)plan.perm_mul;
    W.extra.perm_mod = (int)plan.perm_mod;
    W.extra.row_bound = (int)ix->ntotal;
    const bool track_ovf = ps.nq <= OVF_ROWS;  // per-query overflow flags of this search's slot
    const SearchWorkspace& ws = W;
    for (int64_t qb = 0; qb < ps.nq; qb += MAX_NQ_PER_PASS) {
        const int64_t nq = std::min(MAX_NQ_PER_PASS, ps.nq - qb);
        const int64_t nq_pad = round_up(nq, plan.bn);
        // one launch: queries -> store dtype with zero padded rows / columns, running top-k and counters cleared,
        // thresholds -inf (or seeded from the previous result in a recovery pass), overflow word cleared at the first pass
        // with a query map (recovery of a few queries) workspace row r is row q_map[qb + r] of the caller's arrays
        const int* q_map = ps.q_map ? ps.q_map + qb : nullptr;
        const int64_t row0 = ps.q_map ? 0 : qb;
        W.ovf_q = track_ovf ? ix->ovf_q + (size_t)ps.slot * OVF_ROWS + qb : nullptr;
        const float* margin = ps.band ? ix->x_eps + (size_t)ps.slot * OVF_ROWS + row0 : nullptr;  // BAND pass: seeded k-th exact score - eps
        HIP_OK(launch_search_prepare(ws, (const char*)ps.queries + (size_t)row0 * ix->dim_s * q_es, ps.q_dtype, nq, ix->dim_s,
                                     ix->dtype, nq_pad, ix->dim_pad, qb == 0, recovery > 0 ? ps.out_scores + row0 * k : nullptr,
                                     recovery > 0 ? ps.out_ids + row0 * k : nullptr, k, q_map, stream, margin));
        W.extra.q_label = ps.q_label ? ps.q_label + (size_t)row0 * ps.n_qlab : nullptr;
        W.extra.q_map = q_map;
        for (size_t c = 0; c < plan.stages.size(); ++c) {
            const Stage& sg = plan.stages[c];
            if (launch_stage(ix, W, plan, sg, nq, nq_pad, experiment, stream)) return -1;
            if (ps.band) {
                HIP_OK(launch_exact_rescore(exact_stage_args(ix, ps, ws, row0, sg, c == 0), nq, stream));
                continue;
            }
            int64_t dense_n = -1;
            int flags = c + 1 == plan.stages.size() ? 1 : 0;
            if (sg.kind == ST_DENSE) dense_n = sg.e - sg.b;
            if (sg.kind == ST_GMAX) {
                dense_n = sg.n_groups;
                flags |= 2;
            }
            HIP_OK(launch_select(ws, nq, k, dense_n, flags, stream, ps.id_base, ps.out_scores + row0 * k, ps.out_ids + row0 * k, q_map));
        }
        if (plan.stages.empty())  // empty index: nothing was selected, the cleared top-k leaves as pads
            HIP_OK(launch_output(ws, nq, k, ps.id_base, ps.out_scores + qb * k, ps.out_ids + qb * k, stream));
    }
    if (ps.defer_flags) return 0;
    HIP_OK(hipMemcpyAsync(ix->overflow_host + FLAG_WORDS * ps.slot, ws.overflow, FLAG_WORDS * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipEventRecord(ix->done[ps.slot], stream));
    return 0;
}

int enqueue_search(vodhip_index* ix, const PendingSearch& ps, bool safe, int recovery, hipStream_t stream) {
    const int rc = enqueue_search_impl(ix, ps, safe, recovery, stream);
    // on failure some kernels of this search may already run on buffers the caller is about to release
    if (rc) (void)hipStreamSynchronize(stream);
    return rc;
}

// ---- exact mode (kernels_exact.hip) ----------------------------------------------------------------------------------------
// the scan's list length k' for the caller's k: enough rows that the list usually PROVES itself complete (rows within eps of the
// k-th score: ~5 % more than k for an fp16 store of N(0, 1) x 768 rows, ~70 % more for bf16 x 1024 - profiles/r05_exact_*.json);
// a query whose list does not is searched again as a band pass, so this is a speed knob, never a correctness one
int exact_kx(const vodhip_index* ix, int k, bool upper_limit = false) {
    // upper_limit: what the adaptive list length may grow to when lists keep failing their proof (the bf16 formula, whatever the scan dtype:
    // fp16 at dim 1024 / k 200 needs ~1.3 k, more than its 1.1 k + 16 starting point)
    const int64_t x100 = ix->exact_expand_x100 > 0 ? ix->exact_expand_x100 : ((ix->dtype == VODHIP_F16 && !upper_limit) ? 110 : 200);
    const int64_t kx = ((int64_t)k * x100 + 99) / 100 + 16;
    const int64_t fits = std::max<int64_t>(k, ix->tune.cand_cap / ROW_ALIGN * ROW_ALIGN);  // the scan needs cand_cap >= its list length
    return (int)std::min<int64_t>(std::min<int64_t>(VODHIP_MAX_K, fits), std::max<int64_t>(kx, k));
}

// the scan behind an exact-mode search: same queries, k' results into the slot's list buffers, LOCAL ids
PendingSearch exact_inner(const vodhip_index* ix, const PendingSearch& ps) {
    PendingSearch in = ps;
    in.k = ps.kx;
    in.kx = 0;
    in.id_base = 0;
    in.out_scores = ix->x_list_s[ps.slot];
    in.out_ids = ix->x_list_i[ps.slot];
    in.defer_flags = false;
    return in;
}

// re-score the list of every query of `ps` (LIST mode), then fetch BOTH flag words (the scan's overflow word and the "some query is
// incomplete" word the re-scoring sets: the head of every search pass clears both) and record the slot's event
int enqueue_exact_list(vodhip_index* ix, const PendingSearch& ps, hipStream_t stream) {
    ExactArgs xa;
    xa.plane = ix->data32;
    xa.stride = ix->dim_pad;
    xa.dim = (int)ix->dim;
    xa.dim_pad = (int)ix->dim_pad;
    xa.q_src = ps.queries;
    xa.q_dtype = ps.q_dtype;
    xa.store_dtype = ix->dtype;
    exact_bound_args(ix, xa);
    xa.row_label = (ix->row_label && ps.q_label) ? ix->row_label : nullptr;
    xa.q_label = ps.q_label;
    xa.n_qlab = ps.n_qlab;
    xa.mode = EXACT_LIST;
    xa.list_s = ix->x_list_s[ps.slot];
    xa.list_i = ix->x_list_i[ps.slot];
    xa.kx = ps.kx;
    xa.P = 64;
    while (xa.P < ps.kx + xa.n_out) xa.P <<= 1;
    xa.k = ps.k;
    xa.id_base = ps.id_base;
    xa.out_scores = ps.out_scores;
    xa.out_ids = ps.out_ids;
    xa.eps = ix->x_eps + (size_t)ps.slot * OVF_ROWS;
    xa.flag_word = ix->ws_lane[ps.lane].overflow + 1;
    xa.flag_q = ix->x_flag_q + (size_t)ps.slot * OVF_ROWS;
    HIP_OK(launch_exact_rescore(xa, ps.nq, stream));
    HIP_OK(hipMemcpyAsync(ix->overflow_host + FLAG_WORDS * ps.slot, ix->ws_lane[ps.lane].overflow, FLAG_WORDS * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipEventRecord(ix->done[ps.slot], stream));
    return 0;
}

int exact_reserve_lists(vodhip_index* ix, int slot, size_t elems) {
    if (ix->x_list_cap[slot] >= elems) return 0;
    (void)hipFree(ix->x_list_s[slot]);
    (void)hipFree(ix->x_list_i[slot]);
    ix->x_list_s[slot] = nullptr;
    ix->x_list_i[slot] = nullptr;
    ix->x_list_cap[slot] = 0;
    HIP_OK(hipMalloc((void**)&ix->x_list_s[slot], elems * sizeof(float)));
    HIP_OK(hipMalloc((void**)&ix->x_list_i[slot], elems * sizeof(int64_t)));
    ix->x_list_cap[slot] = elems;
    return 0;
}

// ---- L2 stores (kernels_l2.hip) --------------------------------------------------------------------------------------------
// grow-only; a slot's buffers are idle when it is handed out again (its previous search was finished)
template <typename T>
int l2_reserve(T*& buf, size_t& cap, size_t elems) {
    if (cap >= elems) return 0;
    (void)hipFree(buf);
    buf = nullptr;
    cap = 0;
    HIP_OK(hipMalloc((void**)&buf, elems * sizeof(T)));
    cap = elems;
    return 0;
}

// with "profile": the event `which` of the slot (0 / 1 around the staging launch, 2 / 3 around the first finish launch), recorded now
int l2_profile_mark(vodhip_index* ix, int slot, int which, hipStream_t stream) {
    if (!ix->profile) return 0;
    if (!ix->l2_ev[slot][which]) HIP_OK(hipEventCreate(&ix->l2_ev[slot][which]));
    HIP_OK(hipEventRecord(ix->l2_ev[slot][which], stream));
    return 0;
}

// similarity form -> squared distances in the caller's rows, from the slot's buffers: behind the first pass, and again after recovery
int enqueue_l2_finish(vodhip_index* ix, const PendingSearch& ps, hipStream_t stream) {
    HIP_OK(launch_l2_finish(ix->l2_sim[ps.slot], ix->l2_qn[ps.slot], ps.nq, ps.k, ps.l2_out, stream));
    return 0;
}

// `consume(dev_src, n, r)` is enqueued on `stream` for every slice: rows [r, r + n) of the source, staged at dev_src.  Nothing is waited
// for behind the last slice.  Shared by vodhip_index_add and the host form of vodhip_index_update_rows.
template <class Consume>
int pipeline_host_rows(vodhip_index* ix, const void* rows, int64_t n_rows, int64_t row_bytes, hipStream_t stream, int64_t* pinned_src,
                       Consume&& consume) {
    // Host rows -> HBM, pipelined (round 3; the index is rebuilt every training period, /root/reference/src/vod_exps/recipes/
    // periodic_training.py:53-96, so ingest time is on the trainer's critical path):
    //   pageable source (a NumPy array, an .npy memory map, decoded zarr chunks): CPU threads copy slice i + 1 into a pinned staging
    //   slot while the DMA engine moves slice i and the convert kernel rounds it into the store - two slots, one stream;
    //   pinned / registered source: the DMA reads it in place, no CPU copy at all.
    // Round 2 pushed 64 MB slices of pageable memory through hipMemcpyAsync (staged by the runtime, synchronous) and waited after each.
    hipPointerAttribute_t attr;
    bool src_pinned = false;
    if (hipPointerGetAttributes(&attr, rows) == hipSuccess) src_pinned = attr.type == hipMemoryTypeHost;
    else (void)hipGetLastError();  // an ordinary host pointer is "invalid value" to the runtime: not an error here
    *pinned_src = src_pinned;
    const int64_t rows_per_stage = std::max<int64_t>(1, STAGE_BYTES / row_bytes);
    for (int b = 0; b < 2; ++b) {
        if (!ix->stage_dev[b]) HIP_OK(hipMalloc(&ix->stage_dev[b], STAGE_BYTES));
        if (!src_pinned && !ix->stage_pin[b]) HIP_OK(hipHostMalloc(&ix->stage_pin[b], STAGE_BYTES, hipHostMallocDefault));
        if (!ix->stage_done[b]) HIP_OK(hipEventCreateWithFlags(&ix->stage_done[b], hipEventDisableTiming));
    }
    int n_thr = (int)ix->ingest_threads;
    if (n_thr <= 0) n_thr = (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency()));
    bool used[2] = {false, false};
    int slot = 0;
    for (int64_t r = 0; r < n_rows; r += rows_per_stage, slot ^= 1) {
        const int64_t n = std::min(rows_per_stage, n_rows - r);
        const size_t bytes = (size_t)n * row_bytes;
        const char* src = (const char*)rows + (size_t)r * row_bytes;
        if (used[slot]) HIP_OK(hipEventSynchronize(ix->stage_done[slot]));  // the slot's previous slice has left the staging buffers
        const void* dma_src = src;
        if (!src_pinned) {
            char* dst = (char*)ix->stage_pin[slot];
            const int t_use = (int)std::min<size_t>((size_t)n_thr, std::max<size_t>(1, bytes >> 20));  // >= 1 MB per thread
            if (t_use <= 1) {
                memcpy(dst, src, bytes);
            } else {
                std::vector<std::thread> pool;
                const size_t per = ((bytes + t_use - 1) / t_use + 4095) & ~(size_t)4095;
                for (int t = 0; t < t_use; ++t) {
                    const size_t lo = std::min(bytes, (size_t)t * per), hi = std::min(bytes, lo + per);
                    if (hi > lo) pool.emplace_back([=] { memcpy(dst + lo, src + lo, hi - lo); });
                }
                for (auto& th : pool) th.join();
            }
            dma_src = dst;
        }
        HIP_OK(hipMemcpyAsync(ix->stage_dev[slot], dma_src, bytes, hipMemcpyHostToDevice, stream));
        HIP_OK(consume(ix->stage_dev[slot], n, r));
        HIP_OK(hipEventRecord(ix->stage_done[slot], stream));
        used[slot] = true;
    }
    return 0;
}

// ---- row removal (H2r) -------------------------------------------------------------------------------------------------------------
RemovePlanes store_planes(const vodhip_index* ix) {
    RemovePlanes p;
    p.data = ix->data;
    if (ix->exact) p.data32 = ix->data32, p.row_n2 = ix->row_n2, p.row_d2 = ix->row_d2;
    p.label = ix->row_label;
    p.value = ix->row_value;
    return p;
}

// the bounce buffer carved into the planes the store has now, `*rows` rows each (sections 256-byte aligned)
int ensure_remove_bounce(vodhip_index* ix, hipStream_t stream, RemovePlanes* out, int64_t* rows) {
    const int64_t r = std::min<int64_t>(ix->remove_slab_rows, std::max<int64_t>(1, ix->capacity));
    size_t at = 0;
    auto section = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t o_data = section((size_t)r * ix->dim_pad * 2);
    const size_t o_32 = ix->exact ? section((size_t)r * ix->dim_pad * 4) : 0, o_n2 = ix->exact ? section((size_t)r * 4) : 0, o_d2 = ix->exact ? section((size_t)r * 4) : 0;
    const size_t o_lab = ix->row_label ? section((size_t)r * 4) : 0;
    const size_t o_val = ix->row_value ? section((size_t)r * ix->value_c_pad * 2) : 0;
    if (at > ix->rm_bounce_bytes) {
        HIP_OK(hipStreamSynchronize(stream));  // (launches of an earlier call may still use the old block)
        (void)hipFree(ix->rm_bounce);
        ix->rm_bounce = nullptr;
        ix->rm_bounce_bytes = 0;
        HIP_OK(hipMalloc((void**)&ix->rm_bounce, at));
        ix->rm_bounce_bytes = at;
    }
    char* b = ix->rm_bounce;
    RemovePlanes p;
    p.data = (uint16_t*)(b + o_data);
    if (ix->exact) p.data32 = (float*)(b + o_32), p.row_n2 = (float*)(b + o_n2), p.row_d2 = (float*)(b + o_d2);
    if (ix->row_label) p.label = (int*)(b + o_lab);
    if (ix->row_value) p.value = (uint16_t*)(b + o_val);
    *out = p;
    *rows = r;
    return 0;
}

// rows [src_row, src_row + n) of every plane of `s` -> rows [dst_row, ..) of `d`: contiguous runs, one copy per plane
int copy_plane_rows(const vodhip_index* ix, const RemovePlanes& s, int64_t src_row, const RemovePlanes& d, int64_t dst_row, int64_t n, hipStream_t stream) {
    if (n <= 0) return 0;
    const size_t st = (size_t)ix->dim_pad, cp = (size_t)ix->value_c_pad;
    HIP_OK(hipMemcpyAsync(d.data + (size_t)dst_row * st, s.data + (size_t)src_row * st, (size_t)n * st * 2, hipMemcpyDefault, stream));
    if (s.data32) {
        HIP_OK(hipMemcpyAsync(d.data32 + (size_t)dst_row * st, s.data32 + (size_t)src_row * st, (size_t)n * st * 4, hipMemcpyDefault, stream));
        HIP_OK(hipMemcpyAsync(d.row_n2 + dst_row, s.row_n2 + src_row, (size_t)n * 4, hipMemcpyDefault, stream));
        HIP_OK(hipMemcpyAsync(d.row_d2 + dst_row, s.row_d2 + src_row, (size_t)n * 4, hipMemcpyDefault, stream));
    }
    if (s.label) HIP_OK(hipMemcpyAsync(d.label + dst_row, s.label + src_row, (size_t)n * 4, hipMemcpyDefault, stream));
    if (s.value) HIP_OK(hipMemcpyAsync(d.value + (size_t)dst_row * cp, s.value + (size_t)src_row * cp, (size_t)n * cp * 2, hipMemcpyDefault, stream));
    return 0;
}

// the store now holds `ntotal` rows, fewer than it did: the words that summarise rows, and what lies behind the last row.  The value
// table's pad rows up to round_up(ntotal, 256) are zero again (its documented invariant); the 16-bit rows a scan's last tile may read
// (up to round_up(ntotal, 256) + 512 - the pad of the allocation) are zero as create left them, the labels there match no query.
int remove_set_ntotal(vodhip_index* ix, int64_t ntotal, hipStream_t stream) {
    const int64_t pad_end = std::min<int64_t>(ix->capacity_pad, round_up(ntotal, ROW_ALIGN) + 2 * ROW_ALIGN);
    if (pad_end > ntotal) {
        HIP_OK(hipMemsetAsync(ix->data + (size_t)ntotal * ix->dim_pad, 0, (size_t)(pad_end - ntotal) * ix->dim_pad * 2, stream));
        if (ix->row_label) HIP_OK(hipMemsetAsync(ix->row_label + ntotal, 0xFF, (size_t)(pad_end - ntotal) * sizeof(int), stream));
    }
    if (ix->row_value) {
        const int64_t rows_pad = std::max<int64_t>(1, scan_tiles(ntotal)) * 256;
        if (rows_pad > ntotal) HIP_OK(hipMemsetAsync(ix->row_value + (size_t)ntotal * ix->value_c_pad, 0, (size_t)(rows_pad - ntotal) * ix->value_c_pad * 2, stream));
        ix->value_rows = ntotal;
        ix->value_vmax_ready = false;  // (the column maxima may belong to rows that left)
    }
    if (ix->exact) {  // rows left: the outliers and the two maxima are re-derived before the next search (refresh_exact_stats)
        ix->stats_dirty = true;
        ix->maxima_stale = true;
    }
    ix->ntotal = ntotal;
    return 0;
}

// the caller holds ix->mu, checked the arguments and found no search in flight
int remove_rows_locked(vodhip_index* ix, const int64_t* ids, int64_t row_begin, int64_t n, int location, int64_t id_base, int64_t* new_ids, hipStream_t stream) {
    const bool listed = ids != nullptr;
    const int64_t ntotal = ix->ntotal;
    ix->last_remove[0] = ix->last_remove[1] = ix->last_remove[2] = 0;
    HIP_OK(hipSetDevice(ix->device));
    const int64_t T = remove_tile_rows(ix->remove_slab_rows);
    // listed: any row may leave, the tiles cover the store; a range: they start at the tile of its first row
    const int64_t tile_base = listed ? 0 : row_begin / T * T;
    const int64_t n_tiles = n == 0 ? 0 : (ntotal - tile_base + T - 1) / T;
    if (n == 0 || n_tiles == 0) {  // nothing can leave (an empty call, or a list against an empty store: every slot is skipped)
        ix->last_remove[1] = n;
        return 0;  // (nothing is written, new_ids included: with n == 0 the map is the identity, with no row stored it is empty)
    }
    if (!ix->upd_owner) {
        // (with the two count words of vodhip_index_update_rows, which allocates them together with the table)
        if (!ix->upd_counts) HIP_OK(hipMalloc((void**)&ix->upd_counts, 2 * sizeof(unsigned int)));
        HIP_OK(hipMalloc((void**)&ix->upd_owner, (size_t)std::max<int64_t>(1, ix->capacity) * sizeof(int)));
        // on the call's own stream, and over before anything else uses the table (as in vodhip_index_update_rows)
        HIP_OK(hipMemsetAsync(ix->upd_owner, 0, (size_t)std::max<int64_t>(1, ix->capacity) * sizeof(int), stream));
        HIP_OK(hipStreamSynchronize(stream));
    }
    if (!ix->rm_words) HIP_OK(hipMalloc((void**)&ix->rm_words, RMW_WORDS * sizeof(unsigned int)));
    if (ix->rm_tiles_cap < n_tiles) {
        HIP_OK(hipStreamSynchronize(stream));
        (void)hipFree(ix->rm_tiles);
        ix->rm_tiles = nullptr;
        ix->rm_tiles_cap = 0;
        HIP_OK(hipMalloc((void**)&ix->rm_tiles, (2 * (size_t)n_tiles + 1) * sizeof(int)));
        ix->rm_tiles_cap = n_tiles;
    }
    int* tile_cnt = ix->rm_tiles;
    int* tile_off = ix->rm_tiles + ix->rm_tiles_cap;
    if (listed && location == VODHIP_HOST) {
        if (ix->upd_ids_cap < n) {
            HIP_OK(hipStreamSynchronize(stream));
            (void)hipFree(ix->upd_ids);
            ix->upd_ids = nullptr;
            ix->upd_ids_cap = 0;
            HIP_OK(hipMalloc((void**)&ix->upd_ids, (size_t)n * sizeof(int64_t)));
            ix->upd_ids_cap = n;
        }
        HIP_OK(hipMemcpyAsync(ix->upd_ids, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        ids = ix->upd_ids;
    }
    // MARK, COUNT and SCAN, then the one wait of the call: the host plans the slabs from the tile offsets and learns the new ntotal
    static const unsigned int words0[RMW_WORDS] = {0u, 0u, ~0u, 0u};  // (static: an asynchronous copy may read it after the call returned)
    HIP_OK(hipMemcpyAsync(ix->rm_words, words0, sizeof(words0), hipMemcpyHostToDevice, stream));
    HIP_OK(launch_remove_mark(ids, row_begin, n, id_base, ntotal, ix->upd_owner, ix->rm_words, stream));
    HIP_OK(launch_remove_count_scan(ix->upd_owner, tile_base, T, ntotal, n_tiles, tile_cnt, tile_off, ix->rm_words, stream));
    std::vector<int32_t> off((size_t)n_tiles + 1);
    unsigned int words[RMW_WORDS];
    HIP_OK(hipMemcpyAsync(off.data(), tile_off, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(words, ix->rm_words, sizeof(words), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    const int64_t first_removed = words[RMW_FIRST] == ~0u ? ntotal : (int64_t)words[RMW_FIRST];
    const RemovePlan plan = plan_remove_slabs(off.data(), n_tiles, tile_base, T, ntotal, first_removed, ix->remove_slab_rows);
    ix->last_remove[0] = ntotal - plan.survivors;
    ix->last_remove[1] = words[RMW_SKIPPED];
    ix->last_remove[2] = words[RMW_DUPLICATES];
    if (new_ids) HIP_OK(launch_remove_map(ix->upd_owner, tile_off, tile_base, T, ntotal, new_ids, stream));
    if (plan.survivors == ntotal) return 0;  // every slot was skipped: nothing was marked, nothing is written
    RemoveGatherArgs a;
    a.src = store_planes(ix);
    a.owner = ix->upd_owner;
    a.tile_off = tile_off;
    a.tile_base = tile_base;
    a.tile_rows = (int)T;
    a.stride = ix->dim_pad;
    a.c_pad = ix->value_c_pad;
    a.ntotal = ntotal;
    RemovePlanes bounce;
    int64_t bounce_rows = 0;
    for (const RemoveSlab& s : plan.slabs) {  // in ascending order on the one stream: a slab writes only rows that it or earlier slabs consumed
        a.src_begin = s.src_begin;
        a.src_rows = s.src_rows;
        if (!s.bounced) {
            a.dst = a.src;
            a.dst_sub = 0;
            HIP_OK(launch_remove_gather(a, stream));
            continue;
        }
        if (!bounce_rows && ensure_remove_bounce(ix, stream, &bounce, &bounce_rows)) return -1;
        if (s.n_keep > bounce_rows) return fail("internal: a slab keeps %lld rows, the bounce buffer holds %lld", (long long)s.n_keep, (long long)bounce_rows);
        a.dst = bounce;
        a.dst_sub = s.dst_begin;
        HIP_OK(launch_remove_gather(a, stream));
        if (copy_plane_rows(ix, bounce, 0, a.src, s.dst_begin, s.n_keep, stream)) return -1;
    }
    // FINISH: the owner words of this call back to zero, the pads, the new ntotal
    HIP_OK(hipMemsetAsync(ix->upd_owner + first_removed, 0, (size_t)(ntotal - first_removed) * sizeof(int), stream));
    return remove_set_ntotal(ix, plan.survivors, stream);
}

}  // namespace

namespace vodhip {

int index_remove_move_rows(vodhip_index* src, int64_t src_row, vodhip_index* dst, int64_t dst_row, int64_t n, hipStream_t stream) {
    if (!src || !dst || n < 0 || src_row < 0 || dst_row < 0 || src_row + n > src->capacity || dst_row + n > dst->capacity) return fail("internal: invalid row move");
    if (n == 0) return 0;
    // both shards' planes and the source's bounce buffer are touched: a flat call on a shard's own handle (vodhip_node_index_shard)
    // must not run beside this.  (Address order: two moves in opposite directions cannot lock each other out.)
    std::unique_lock<std::mutex> lock_a(src < dst ? src->mu : dst->mu), lock_b;
    if (src != dst) lock_b = std::unique_lock<std::mutex>(src < dst ? dst->mu : src->mu);
    const RemovePlanes s = store_planes(src), d = store_planes(dst);
    if (src->dim_pad != dst->dim_pad || (s.data32 != nullptr) != (d.data32 != nullptr) || (s.label != nullptr) != (d.label != nullptr) ||
        (s.value != nullptr) != (d.value != nullptr) || src->value_c_pad != dst->value_c_pad)
        return fail("internal: the shards of a row move do not keep the same planes");
    if (s.value && (dst_row + n > dst->value_alloc_rows || src_row + n > src->value_alloc_rows)) return fail("internal: a value table is too short for the row move");
    HIP_OK(hipSetDevice(dst->device));
    if (src != dst || dst_row + n <= src_row || src_row + n <= dst_row) {
        if (copy_plane_rows(src, s, src_row, d, dst_row, n, stream)) return -1;
    } else {  // one shard, the destination covers part of the source: in ascending pieces through the bounce buffer
        if (dst_row > src_row) return fail("internal: a row move upwards");
        RemovePlanes bounce;
        int64_t bounce_rows = 0;
        if (ensure_remove_bounce(src, stream, &bounce, &bounce_rows)) return -1;
        for (int64_t r = 0; r < n; r += bounce_rows) {
            const int64_t m = std::min(bounce_rows, n - r);
            if (copy_plane_rows(src, s, src_row + r, bounce, 0, m, stream)) return -1;
            if (copy_plane_rows(src, bounce, 0, d, dst_row + r, m, stream)) return -1;
        }
    }
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
}

int index_remove_set_ntotal(vodhip_index* ix, int64_t ntotal, hipStream_t stream) {
    if (!ix || ntotal < 0 || ntotal > ix->capacity) return fail("internal: invalid ntotal");
    std::lock_guard<std::mutex> guard(ix->mu);
    HIP_OK(hipSetDevice(ix->device));
    if (remove_set_ntotal(ix, ntotal, stream)) return -1;
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
}

}  // namespace vodhip

extern "C" {

const char* vodhip_last_error(void) { return g_last_error.c_str(); }
int vodhip_version(void) { return VODHIP_VERSION; }

int vodhip_index_create(int device, int64_t dim, int store_dtype, int64_t capacity_rows, vodhip_index_t** out) {
    if (!out) return fail("out is NULL");
    if (dim <= 0 || capacity_rows < 0) return fail("invalid dim=%lld / capacity=%lld", (long long)dim, (long long)capacity_rows);
    const bool exact = (store_dtype & VODHIP_EXACT_F32) != 0;
    const bool l2 = (store_dtype & VODHIP_L2) != 0;
    store_dtype &= ~(VODHIP_EXACT_F32 | VODHIP_L2);
    if (store_dtype != VODHIP_F16 && store_dtype != VODHIP_BF16) return fail("store dtype must be F16 or BF16 (optionally | VODHIP_EXACT_F32 or | VODHIP_L2)");
    if (l2 && exact) return fail("VODHIP_L2 | VODHIP_EXACT_F32 is not supported: an L2 store scores the rounded rows (DESIGN.md 8)");
    if (exact && (dim + 63) / 64 * 64 > 16384) return fail("VODHIP_EXACT_F32 stores take dim <= 16384");
    if (capacity_rows >= (1ll << 31) - 2 * ROW_ALIGN) return fail("capacity must be < 2^31 rows per device");
    HIP_OK(hipSetDevice(device));
    vodhip_index* ix = new vodhip_index();
    ix->device = device;
    ix->dim = dim;
    ix->l2 = l2;
    ix->dim_s = l2 ? dim + L2_BIAS_COLS : dim;
    ix->dim_pad = round_up(ix->dim_s, 64);
    ix->capacity = capacity_rows;
    ix->capacity_pad = round_up(capacity_rows, ROW_ALIGN) + 2 * ROW_ALIGN;  // the last tile (up to 384 rows from a 256-aligned start) never reads past the allocation
    ix->dtype = store_dtype;
    ix->exact = exact;
    if (hipDeviceGetAttribute(&ix->tune.n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ix->tune.n_cu < 1) ix->tune.n_cu = 256;
    ix->ws_lane[0].n_cu = ix->ws_lane[1].n_cu = ix->tune.n_cu;
    const size_t bytes = (size_t)ix->capacity_pad * ix->dim_pad * 2;
    hipError_t e = hipMalloc((void**)&ix->data, bytes);
    if (e != hipSuccess) {
        delete ix;
        return fail("hipMalloc of the %zu-byte vector store failed: %s", bytes, hipGetErrorString(e));
    }
    e = hipMemset(ix->data, 0, bytes);
    // hipMemset of device memory returns before the fill has run; rows are ingested (and searched) on streams that do not order
    // themselves behind the null stream (the batcher's and the node index's are non-blocking): the fill must be over before any of that
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = hipMalloc((void**)&ix->ovf_q, MAX_IN_FLIGHT * OVF_ROWS * sizeof(unsigned int));
    if (e == hipSuccess) e = hipMalloc((void**)&ix->q_map, MAX_IN_FLIGHT * OVF_ROWS * sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc((void**)&ix->overflow_host, FLAG_WORDS * MAX_IN_FLIGHT * sizeof(unsigned int), hipHostMallocDefault);
    for (int i = 0; i < MAX_IN_FLIGHT && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ix->done[i], hipEventDisableTiming);
    for (int i = 0; i < MAX_IN_FLIGHT && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ix->lane_in[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ix->lane_stream, hipStreamNonBlocking);
    if (l2 && e == hipSuccess) e = hipMalloc((void**)&ix->l2_sat, sizeof(unsigned int));
    if (l2 && e == hipSuccess) e = hipMemset(ix->l2_sat, 0, sizeof(unsigned int));
    if (l2 && e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (exact && e == hipSuccess) {
        // the float32 plane (rows are written whole, zero padded columns included: no fill needed) + the bound's bookkeeping
        const size_t bytes32 = ((size_t)capacity_rows + 1) * ix->dim_pad * sizeof(float);
        e = hipMalloc((void**)&ix->data32, bytes32);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(ix->data);
            (void)hipFree(ix->ovf_q);
            (void)hipFree(ix->q_map);
            (void)hipHostFree(ix->overflow_host);
            delete ix;
            return fail("hipMalloc of the %zu-byte float32 plane (VODHIP_EXACT_F32) failed: %s", bytes32, hipGetErrorString(e));
        }
        if (e == hipSuccess) e = hipMalloc((void**)&ix->norm_stats, EXS_WORDS * sizeof(unsigned int));
        if (e == hipSuccess) e = hipMemset(ix->norm_stats, 0, EXS_WORDS * sizeof(unsigned int));
        if (e == hipSuccess) e = hipMalloc((void**)&ix->row_n2, ((size_t)capacity_rows + 1) * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&ix->row_d2, ((size_t)capacity_rows + 1) * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&ix->x_eps, MAX_IN_FLIGHT * OVF_ROWS * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void**)&ix->x_flag_q, MAX_IN_FLIGHT * OVF_ROWS * sizeof(unsigned int));
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(ix->data);
        (void)hipFree(ix->data32);
        (void)hipFree(ix->l2_sat);
        delete ix;
        return fail("store initialisation failed: %s", hipGetErrorString(e));
    }
    for (int i = 0; i < FLAG_WORDS * MAX_IN_FLIGHT; ++i) ix->overflow_host[i] = 0;
    *out = ix;
    return 0;
}

int vodhip_index_destroy(vodhip_index_t* ix) {
    if (!ix) return 0;
    (void)hipSetDevice(ix->device);
    if (!ix->inflight.empty()) (void)hipDeviceSynchronize();  // enqueued searches still use the store and the workspace
    free_workspace(ix, 0);
    free_workspace(ix, 1);
    if (ix->lane_stream) (void)hipStreamDestroy(ix->lane_stream);
    for (int i = 0; i < MAX_IN_FLIGHT; ++i)
        if (ix->lane_in[i]) (void)hipEventDestroy(ix->lane_in[i]);
    for (hipEvent_t e : ix->ev_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < MAX_IN_FLIGHT; ++i)
        if (ix->done[i]) (void)hipEventDestroy(ix->done[i]);
    (void)hipFree(ix->data);
    for (int b = 0; b < 2; ++b) {
        (void)hipFree(ix->stage_dev[b]);
        (void)hipHostFree(ix->stage_pin[b]);
        if (ix->stage_done[b]) (void)hipEventDestroy(ix->stage_done[b]);
    }
    (void)hipFree(ix->data32);
    (void)hipFree(ix->norm_stats);
    (void)hipFree(ix->row_n2);
    (void)hipFree(ix->row_d2);
    (void)hipFree(ix->x_eps);
    (void)hipFree(ix->x_flag_q);
    for (int i = 0; i < MAX_IN_FLIGHT; ++i) {
        (void)hipFree(ix->x_list_s[i]);
        (void)hipFree(ix->x_list_i[i]);
    }
    (void)hipFree(ix->l2_sat);
    (void)hipFree(ix->upd_owner);
    (void)hipFree(ix->upd_counts);
    (void)hipFree(ix->upd_ids);
    (void)hipFree(ix->rm_words);
    (void)hipFree(ix->rm_tiles);
    (void)hipFree(ix->rm_bounce);
    for (int i = 0; i < MAX_IN_FLIGHT; ++i)
        for (hipEvent_t e : ix->l2_ev[i])
            if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < MAX_IN_FLIGHT; ++i) {
        (void)hipFree(ix->l2_q[i]);
        (void)hipFree(ix->l2_qn[i]);
        (void)hipFree(ix->l2_sim[i]);
    }
    (void)hipFree(ix->row_label);
    (void)hipFree(ix->row_value);
    (void)hipFree(ix->value_vmax);
    (void)hipFree(ix->sample_ws);
    (void)hipFree(ix->ovf_q);
    (void)hipFree(ix->q_map);
    (void)hipHostFree(ix->overflow_host);
    delete ix;
    return 0;
}

int vodhip_index_add(vodhip_index_t* ix, const void* rows, int64_t n_rows, int src_dtype, int src_location, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (n_rows < 0 || (n_rows > 0 && !rows)) return fail("invalid rows");
    if (src_dtype < 0 || src_dtype > 2) return fail("invalid src_dtype %d", src_dtype);
    if (ix->ntotal + n_rows > ix->capacity)
        return fail("index full: ntotal=%lld + %lld > capacity=%lld", (long long)ix->ntotal, (long long)n_rows, (long long)ix->capacity);
    if (!ix->inflight.empty()) return fail("%d searches are in flight: finish them before adding rows", (int)ix->inflight.size());
    hipStream_t stream = (hipStream_t)stream_;
    HIP_OK(hipSetDevice(ix->device));
    ix->stats_dirty = true;  // exact mode: the bound's maxima / outliers are re-derived before the next search
    const int es = elem_size(src_dtype);
    // one launch per slice: the rounded plane, and for VODHIP_EXACT_F32 stores also the float32 plane + the row statistics
    auto ingest = [&](const void* dev_src, int64_t n, int64_t first_row) -> hipError_t {
        if (ix->exact)
            return launch_ingest_exact(dev_src, src_dtype, n, ix->dim, ix->data + (size_t)first_row * ix->dim_pad, ix->dtype,
                                       ix->data32 + (size_t)first_row * ix->dim_pad, ix->dim_pad, ix->norm_stats, ix->row_n2 + first_row,
                                       ix->row_d2 + first_row, stream);
        hipError_t e = launch_convert_rows(dev_src, src_dtype, n, ix->dim, ix->data + (size_t)first_row * ix->dim_pad, ix->dtype, ix->dim_pad, stream);
        // L2 store: the bias columns, from the values as stored (one more launch per slice, behind the conversion)
        if (e == hipSuccess && ix->l2)
            e = launch_l2_bias(ix->data + (size_t)first_row * ix->dim_pad, ix->dtype, n, ix->dim, ix->dim_pad, ix->l2_sat, stream);
        return e;
    };
    if (src_location == VODHIP_DEVICE) {
        HIP_OK(ingest(rows, n_rows, ix->ntotal));
        ix->ntotal += n_rows;
        return 0;
    }
    if (src_location != VODHIP_HOST) return fail("invalid src_location %d", src_location);
    int64_t src_pinned = 0;
    const int rc = pipeline_host_rows(ix, rows, n_rows, ix->dim * es, stream, &src_pinned,
                                      [&](const void* dev_src, int64_t n, int64_t r) { return ingest(dev_src, n, ix->ntotal + r); });
    ix->last_ingest_pinned_src = src_pinned;
    if (rc) return -1;
    HIP_OK(hipStreamSynchronize(stream));  // synchronous for host sources: the caller may free `rows` on return
    ix->ntotal += n_rows;
    return 0;
}

// H2u: listed or contiguous stored rows changed in place (kernels_update.hip); ntotal, the labels and the value table stay
int vodhip_index_update_rows(vodhip_index_t* ix, const int64_t* ids, int64_t row_begin, const void* rows, int64_t n, int src_dtype, int location,
                             int mode, float alpha, int64_t id_base, void* stream_) {
    if (!ix) return fail("index is NULL");
    std::lock_guard<std::mutex> guard(ix->mu);
    if (const char* msg = update_rows_args_error(ids != nullptr, row_begin, rows, n, src_dtype, location, mode, alpha, ix->ntotal)) {
        if (!strcmp(msg, "invalid src_dtype")) return fail("invalid src_dtype %d", src_dtype);
        if (!strcmp(msg, "invalid location")) return fail("invalid location %d", location);
        if (!strcmp(msg, "invalid mode")) return fail("invalid mode %d", mode);
        if (!strncmp(msg, "alpha", 5)) return fail("alpha=%g: %s", (double)alpha, msg);
        if (!strncmp(msg, "row range", 9)) return fail("rows [%lld, %lld + %lld), ntotal=%lld: %s", (long long)row_begin, (long long)row_begin, (long long)n, (long long)ix->ntotal, msg);
        return fail("n=%lld: %s", (long long)n, msg);
    }
    if (!ix->inflight.empty() || ix->unfinished)
        return fail("%d searches are in flight: finish them before updating rows", (int)ix->inflight.size() + ix->unfinished);
    const bool listed = ids != nullptr;
    ix->last_update_n = n;
    ix->last_update_listed = listed && n > 0;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_OK(hipSetDevice(ix->device));
    if (listed && !ix->upd_owner) {
        int* owner = nullptr;
        HIP_OK(hipMalloc((void**)&owner, (size_t)std::max<int64_t>(1, ix->capacity) * sizeof(int)));
        if (hipError_t e = hipMalloc((void**)&ix->upd_counts, 2 * sizeof(unsigned int)); e != hipSuccess) {
            (void)hipFree(owner);
            return fail("hipMalloc failed: %s", hipGetErrorString(e));
        }
        ix->upd_owner = owner;
        // on the call's own stream, and over before anything else uses the table (the rule of the label fill in set_row_labels)
        HIP_OK(hipMemsetAsync(ix->upd_owner, 0, (size_t)std::max<int64_t>(1, ix->capacity) * sizeof(int), stream));
        HIP_OK(hipStreamSynchronize(stream));
    }
    if (ix->exact) {  // the outliers and - since rows LEFT - the two maxima are re-derived before the next search (refresh_exact_stats)
        ix->stats_dirty = true;
        ix->maxima_stale = true;
    }
    UpdateArgs a;
    a.src_dtype = src_dtype;
    a.row_begin = row_begin;
    a.id_base = id_base;
    a.ntotal = ix->ntotal;
    a.dim = ix->dim;
    a.stride = ix->dim_pad;
    a.store_dtype = ix->dtype;
    a.kind = ix->exact ? UPDATE_EXACT : ix->l2 ? UPDATE_L2 : UPDATE_PLAIN;
    a.mode = mode;
    a.alpha = alpha;
    a.data = ix->data;
    a.data32 = ix->data32;
    a.row_n2 = ix->row_n2;
    a.row_d2 = ix->row_d2;
    a.norm_stats = ix->norm_stats;
    a.l2_sat = ix->l2_sat;
    a.owner = ix->upd_owner;
    a.counts = ix->upd_counts;
    if (listed) HIP_OK(hipMemsetAsync(ix->upd_counts, 0, 2 * sizeof(unsigned int), stream));
    if (location == VODHIP_DEVICE) {
        a.ids = ids;
        a.src = rows;
        a.n_slots = n;
        if (listed) HIP_OK(launch_update_claim(ids, n, id_base, ix->ntotal, ix->upd_owner, stream));
        HIP_OK(launch_update_rows(a, stream));
        return 0;
    }
    // host source: the ids go up once and are claimed once - duplicates are resolved over the whole call, not per slice - then the rows
    // go through the ingest pipeline's staging slots, one write launch per slice
    if (listed) {
        if (ix->upd_ids_cap < n) {
            HIP_OK(hipStreamSynchronize(stream));
            (void)hipFree(ix->upd_ids);
            ix->upd_ids = nullptr;
            ix->upd_ids_cap = 0;
            HIP_OK(hipMalloc((void**)&ix->upd_ids, (size_t)n * sizeof(int64_t)));
            ix->upd_ids_cap = n;
        }
        HIP_OK(hipMemcpyAsync(ix->upd_ids, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        HIP_OK(launch_update_claim(ix->upd_ids, n, id_base, ix->ntotal, ix->upd_owner, stream));
        a.ids = ix->upd_ids;
    }
    int64_t src_pinned = 0;
    const int rc = pipeline_host_rows(ix, rows, n, ix->dim * elem_size(src_dtype), stream, &src_pinned, [&](const void* dev_src, int64_t cnt, int64_t r) {
        a.src = dev_src;
        a.slot_begin = r;
        a.n_slots = cnt;
        return launch_update_rows(a, stream);
    });
    // (also after a failure: launches of this call may still read the staging slots, and the owner table must be back to zero before
    // the next call - a slice that never ran leaves its claims behind)
    hipError_t e = hipStreamSynchronize(stream);
    if (rc != 0 && listed) {
        if (e == hipSuccess) e = hipMemsetAsync(ix->upd_owner, 0, (size_t)std::max<int64_t>(1, ix->capacity) * sizeof(int), stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
    }
    if (rc) return -1;
    HIP_OK(e);
    return 0;
}

// H2r: listed or contiguous stored rows removed, the survivors moved down in order (kernels_remove.hip, remove_fold.h)
int vodhip_index_remove_rows(vodhip_index_t* ix, const int64_t* ids, int64_t row_begin, int64_t n, int location, int64_t id_base, int64_t* new_ids,
                             int64_t* n_removed, void* stream_) {
    if (!ix) return fail("index is NULL");
    std::lock_guard<std::mutex> guard(ix->mu);
    if (const char* msg = remove_rows_args_error(ids != nullptr, row_begin, n, location, ix->ntotal)) {
        if (!strcmp(msg, "invalid location")) return fail("invalid location %d", location);
        if (!strncmp(msg, "row range", 9)) return fail("rows [%lld, %lld + %lld), ntotal=%lld: %s", (long long)row_begin, (long long)row_begin, (long long)n, (long long)ix->ntotal, msg);
        return fail("n=%lld: %s", (long long)n, msg);
    }
    if (!ix->inflight.empty() || ix->unfinished)
        return fail("%d searches are in flight: finish them before removing rows", (int)ix->inflight.size() + ix->unfinished);
    // a table left short by rows added after it was set describes other rows than the store holds (every read-out refuses it): moving
    // it with the rows would read past its allocation and then pass it off as valid
    if (ix->row_value && ix->value_rows != ix->ntotal)
        return fail("remove_rows: the value table holds %lld rows, the index %lld: set the table again (or clear it) after adding rows, then remove",
                    (long long)ix->value_rows, (long long)ix->ntotal);
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = remove_rows_locked(ix, ids, row_begin, n, location, id_base, new_ids, stream);
    if (rc != 0 && ix->upd_owner) {
        // whatever the call marked must not outlive it: update_rows and the next removal read the table as all zero.  (Best effort,
        // the error text of the failure is kept.)
        (void)hipStreamSynchronize(stream);
        (void)hipMemsetAsync(ix->upd_owner, 0, (size_t)std::max<int64_t>(1, ix->capacity) * sizeof(int), stream);
        (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
    }
    if (rc == 0 && n_removed) *n_removed = ix->last_remove[0];
    return rc;
}

int vodhip_index_reset(vodhip_index_t* ix) {
    if (!ix) return fail("index is NULL");
    if (!ix->inflight.empty()) return fail("%d searches are in flight: finish them before resetting the index", (int)ix->inflight.size());
    if (ix->exact) {  // the row maxima of the error bound start over with the store (stale maxima would only loosen it)
        HIP_OK(hipSetDevice(ix->device));
        HIP_OK(hipDeviceSynchronize());  // ingests of the old rows may still run on some stream
        HIP_OK(hipMemset(ix->norm_stats, 0, EXS_WORDS * sizeof(unsigned int)));
        HIP_OK(hipStreamSynchronize(nullptr));
        ix->stats_dirty = true;
        ix->maxima_stale = false;  // (the words were just cleared)
        ix->adapt_k = ix->adapt_kx = 0;
    }
    if (ix->l2) {  // the saturation count starts over with the store
        HIP_OK(hipSetDevice(ix->device));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemset(ix->l2_sat, 0, sizeof(unsigned int)));
        HIP_OK(hipStreamSynchronize(nullptr));
    }
    if (ix->row_value) {  // the value table describes the rows that leave
        HIP_OK(hipSetDevice(ix->device));
        HIP_OK(hipDeviceSynchronize());  // a read-out of the old rows may still run on some stream
        (void)hipFree(ix->row_value);
        (void)hipFree(ix->value_vmax);
        ix->row_value = nullptr;
        ix->value_vmax = nullptr;
        ix->value_vmax_ready = false;
        ix->value_rows = ix->value_cols = ix->value_c_pad = 0;
    }
    ix->ntotal = 0;
    return 0;
}

int vodhip_index_ntotal(const vodhip_index_t* ix, int64_t* out) {
    if (!ix || !out) return fail("NULL argument");
    *out = ix->ntotal;
    return 0;
}
int vodhip_index_dim(const vodhip_index_t* ix, int64_t* out) {
    if (!ix || !out) return fail("NULL argument");
    *out = ix->dim;
    return 0;
}
int vodhip_index_capacity(const vodhip_index_t* ix, int64_t* out) {
    if (!ix || !out) return fail("NULL argument");
    *out = ix->capacity;
    return 0;
}
int vodhip_index_data(const vodhip_index_t* ix, void** dev_ptr, int64_t* row_stride_elems, int* store_dtype) {
    if (!ix) return fail("index is NULL");
    if (dev_ptr) *dev_ptr = ix->data;
    if (row_stride_elems) *row_stride_elems = ix->dim_pad;
    if (store_dtype) *store_dtype = ix->dtype;
    return 0;
}

int vodhip_index_get_rows(const vodhip_index_t* ix, int64_t row_begin, int64_t n_rows, void* dst, int dst_location,
                          void* stream_) {
    if (!ix) return fail("index is NULL");
    if (row_begin < 0 || n_rows < 0 || row_begin + n_rows > ix->ntotal) return fail("row range out of bounds");
    if (n_rows == 0) return 0;
    if (!dst) return fail("dst is NULL");
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    const hipMemcpyKind kind = dst_location == VODHIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIP_OK(hipMemcpy2DAsync(dst, (size_t)ix->dim * 2, ix->data + (size_t)row_begin * ix->dim_pad, (size_t)ix->dim_pad * 2,
                            (size_t)ix->dim * 2, (size_t)n_rows, kind, stream));
    if (dst_location != VODHIP_DEVICE) HIP_OK(hipStreamSynchronize(stream));
    return 0;
}

int vodhip_index_data_f32(const vodhip_index_t* ix, void** dev_ptr, int64_t* row_stride_elems) {
    if (!ix) return fail("index is NULL");
    if (!ix->exact) return fail("the index was not created with VODHIP_EXACT_F32: it keeps no float32 rows");
    if (dev_ptr) *dev_ptr = ix->data32;
    if (row_stride_elems) *row_stride_elems = ix->dim_pad;
    return 0;
}

int vodhip_index_plane(const vodhip_index_t* ix, int which, void** dev_ptr, int64_t* n_rows, int64_t* row_stride_elems) {
    if (!ix) return fail("index is NULL");
    void* p = nullptr;
    int64_t rows = ix->ntotal, stride = 1;
    switch (which) {
        case VODHIP_PLANE_LABELS: p = ix->row_label; break;
        case VODHIP_PLANE_VALUES:
            p = ix->row_value;
            rows = ix->row_value ? std::max<int64_t>(1, scan_tiles(ix->value_rows)) * 256 : 0;
            stride = ix->value_c_pad;
            break;
        case VODHIP_PLANE_ROW_N2: p = ix->row_n2; break;
        case VODHIP_PLANE_ROW_D2: p = ix->row_d2; break;
        case VODHIP_PLANE_OWNER:
            p = ix->upd_owner;
            rows = ix->upd_owner ? std::max<int64_t>(1, ix->capacity) : 0;
            break;
        default: return fail("invalid plane %d", which);
    }
    if (!p) rows = 0;
    if (dev_ptr) *dev_ptr = p;
    if (n_rows) *n_rows = rows;
    if (row_stride_elems) *row_stride_elems = stride;
    return 0;
}

int vodhip_index_get_rows_f32(const vodhip_index_t* ix, int64_t row_begin, int64_t n_rows, void* dst, int dst_location, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (!ix->exact) return fail("the index was not created with VODHIP_EXACT_F32: it keeps no float32 rows");
    if (row_begin < 0 || n_rows < 0 || row_begin + n_rows > ix->ntotal) return fail("row range out of bounds");
    if (n_rows == 0) return 0;
    if (!dst) return fail("dst is NULL");
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    const hipMemcpyKind kind = dst_location == VODHIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIP_OK(hipMemcpy2DAsync(dst, (size_t)ix->dim * 4, ix->data32 + (size_t)row_begin * ix->dim_pad, (size_t)ix->dim_pad * 4,
                            (size_t)ix->dim * 4, (size_t)n_rows, kind, stream));
    if (dst_location != VODHIP_DEVICE) HIP_OK(hipStreamSynchronize(stream));
    return 0;
}

int vodhip_index_set_row_labels(vodhip_index_t* ix, const int32_t* labels, int64_t n_rows, int location, void* stream_) {
    if (!ix) return fail("index is NULL");
    std::lock_guard<std::mutex> guard(ix->mu);
    // searches in flight read the labels - on the caller's stream or, with two lanes, on the index's own: like add / reset, refuse
    // (round-5 advisor: a lane-1 subset search could still be reading `row_label` while this call overwrote / freed it)
    if (!ix->inflight.empty() || ix->unfinished) return fail("%d searches are in flight: finish them before changing the row labels", (int)ix->inflight.size() + ix->unfinished);
    HIP_OK(hipSetDevice(ix->device));
    if (!labels) {  // clear
        (void)hipFree(ix->row_label);
        ix->row_label = nullptr;
        return 0;
    }
    if (n_rows < 0 || n_rows > ix->capacity) return fail("n_rows=%lld out of range", (long long)n_rows);
    hipStream_t stream = (hipStream_t)stream_;
    if (!ix->row_label) {
        HIP_OK(hipMalloc((void**)&ix->row_label, (size_t)ix->capacity_pad * sizeof(int)));
        // -1: matches no query label.  On the SAME stream as the copy below: a null-stream hipMemset is not ordered before work on a
        // non-blocking stream (the node index's shard streams), and the late fill wiped the labels just copied - every restricted query
        // of the FIRST filtered search of a process came back empty (round 4, fuzz_search seed 404 trial 1051: found, fixed, pinned by
        // tests/test_node_index_gpu.py::test_row_labels_set_on_a_non_blocking_stream_survive_the_initial_fill)
        HIP_OK(hipMemsetAsync(ix->row_label, 0xFF, (size_t)ix->capacity_pad * sizeof(int), stream));
    }
    HIP_OK(hipMemcpyAsync(ix->row_label, labels, (size_t)n_rows * sizeof(int),
                          location == VODHIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
}

// the value table of vodhip_index_posterior_expectation: converted to the store dtype on the device, pad columns and pad rows zero
int vodhip_index_set_row_values(vodhip_index_t* ix, const void* values, int64_t n_rows, int64_t n_cols, int src_dtype, int location, void* stream_) {
    if (!ix) return fail("index is NULL");
    std::lock_guard<std::mutex> guard(ix->mu);
    if (!ix->inflight.empty() || ix->unfinished) return fail("%d searches are in flight: finish them before changing the row values", (int)ix->inflight.size() + ix->unfinished);
    if (values) {
        if (const char* msg = row_values_args_error(n_rows, n_cols, src_dtype, location, ix->ntotal)) {
            if (!strcmp(msg, "invalid src_dtype")) return fail("invalid src_dtype %d", src_dtype);
            if (!strcmp(msg, "invalid location")) return fail("invalid location %d", location);
            if (msg[2] == 'c') return fail("n_cols=%lld: %s (wider tables are not supported)", (long long)n_cols, msg);
            return fail("n_rows=%lld, ntotal=%lld: %s", (long long)n_rows, (long long)ix->ntotal, msg);
        }
    }
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    HIP_OK(hipDeviceSynchronize());  // a read-out of the old table may still run on some stream (as in vodhip_index_reset)
    (void)hipFree(ix->row_value);
    (void)hipFree(ix->value_vmax);
    ix->row_value = nullptr;
    ix->value_vmax = nullptr;
    ix->value_vmax_ready = false;
    ix->value_rows = ix->value_cols = ix->value_c_pad = 0;
    if (!values) return 0;
    const int64_t c_pad = readout_c_pad(n_cols);
    const int64_t rows_pad = std::max<int64_t>(1, scan_tiles(n_rows)) * 256;
    uint16_t* table = nullptr;
    HIP_OK(hipMalloc((void**)&table, (size_t)rows_pad * (size_t)c_pad * 2));
    auto fill = [&]() -> hipError_t {
        if (n_rows < rows_pad)
            if (hipError_t e = hipMemsetAsync(table + (size_t)n_rows * c_pad, 0, (size_t)(rows_pad - n_rows) * (size_t)c_pad * 2, stream); e != hipSuccess) return e;
        if (n_rows == 0) return hipSuccess;
        const void* src = values;
        void* staged = nullptr;
        if (location == VODHIP_HOST) {
            const size_t bytes = (size_t)n_rows * (size_t)n_cols * (size_t)elem_size(src_dtype);
            if (hipError_t e = hipMalloc(&staged, bytes); e != hipSuccess) return e;
            if (hipError_t e = hipMemcpyAsync(staged, values, bytes, hipMemcpyHostToDevice, stream); e != hipSuccess) {
                (void)hipFree(staged);
                return e;
            }
            src = staged;
        }
        hipError_t e = launch_convert_rows(src, src_dtype, n_rows, n_cols, table, ix->dtype, c_pad, stream);
        const hipError_t se = hipStreamSynchronize(stream);
        if (staged) (void)hipFree(staged);
        return e != hipSuccess ? e : se;
    };
    if (hipError_t e = fill(); e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(table);
        return fail("building the row-value table failed: %s", hipGetErrorString(e));
    }
    ix->row_value = table;
    ix->value_alloc_rows = rows_pad;
    ix->value_rows = n_rows;
    ix->value_cols = n_cols;
    ix->value_c_pad = c_pad;
    return 0;
}

int vodhip_index_row_values_info(const vodhip_index_t* ix, int64_t* n_rows, int64_t* n_cols) {
    if (!ix) return fail("index is NULL");
    if (n_rows) *n_rows = ix->row_value ? ix->value_rows : 0;
    if (n_cols) *n_cols = ix->row_value ? ix->value_cols : 0;
    return 0;
}

int vodhip_index_set_query_labels(vodhip_index_t* ix, const int32_t* q_labels_dev, int n_per_query) {
    if (!ix) return fail("index is NULL");
    if (q_labels_dev && (n_per_query < 1 || n_per_query > 64)) return fail("n_per_query must be in [1, 64]");
    if (q_labels_dev && !ix->row_label) return fail("set the row labels first (vodhip_index_set_row_labels)");
    std::lock_guard<std::mutex> guard(ix->mu);
    ix->q_label = q_labels_dev;
    ix->n_qlab = q_labels_dev ? n_per_query : 0;
    return 0;
}

int vodhip_index_search_async(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, int k, int64_t id_base,
                              float* out_scores, int64_t* out_ids, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (k < 1 || k > VODHIP_MAX_K) return fail("k=%d out of range [1, %d]", k, VODHIP_MAX_K);
    if (nq < 0 || (nq > 0 && (!queries || !out_scores || !out_ids))) return fail("invalid query / output pointers");
    if (q_dtype < 0 || q_dtype > 2) return fail("invalid q_dtype %d", q_dtype);
    std::lock_guard<std::mutex> guard(ix->mu);
    if (ix->tune.cand_cap < ROW_ALIGN || ix->tune.cand_cap < k) return fail("cand_cap too small");
    if ((int)ix->inflight.size() + ix->unfinished >= MAX_IN_FLIGHT)
        return fail("%d searches are already in flight on this index: call vodhip_index_search_finish first", MAX_IN_FLIGHT);
    if (ix->exact && nq > OVF_ROWS) return fail("VODHIP_EXACT_F32: at most %lld queries per search", (long long)OVF_ROWS);
    HIP_OK(hipSetDevice(ix->device));
    PendingSearch ps;
    ps.active = true;
    ps.queries = queries;
    ps.q_dtype = q_dtype;
    ps.nq = nq;
    ps.k = k;
    ps.id_base = id_base;
    ps.out_scores = out_scores;
    ps.out_ids = out_ids;
    ps.q_label = ix->q_label;
    ps.n_qlab = ix->n_qlab;
    ps.slot = ix->next_slot;
    // lane: batches of one query tile alternate between the two workspaces (auto), so that a caller running one search ahead has two
    // searches on the device at once; lane 1 runs on the index's own stream, behind what the caller's stream holds now (the queries)
    hipStream_t stream = (hipStream_t)stream_;
    if (ix->exact && nq > 0 && refresh_exact_stats(ix, stream)) return -1;
    const int64_t lanes_eff = ix->lanes > 0 ? ix->lanes : (nq <= 256 ? 2 : 1);
    if (lanes_eff == 2 && nq > 0) {
        // the lane the youngest search in flight does NOT use; a caller that finishes every search before the next (nothing in flight)
        // stays on lane 0 = its own stream, with no event hop
        ps.lane = ix->inflight.empty() ? 0 : 1 - ix->inflight.back().lane;
        if (ps.lane == 1) {
            HIP_OK(hipEventRecord(ix->lane_in[ps.slot], stream));
            HIP_OK(hipStreamWaitEvent(ix->lane_stream, ix->lane_in[ps.slot], 0));
            stream = ix->lane_stream;
        }
    }
    if (ix->inflight.empty() && ix->unfinished == 0) ix->ev_used = 0;  // profile events are recycled once nothing refers to them
    ps.ev_begin = ix->ev_used;
    if (ix->l2 && nq > 0) {
        // L2 store: ONE staging launch (rounded queries + the three constants, |q~|^2), the unchanged search over dim + 3 columns
        // into the slot's similarity-form buffer, ONE finish launch into the caller's scores, then the flag words: no host round trip
        if (l2_reserve(ix->l2_q[ps.slot], ix->l2_q_cap[ps.slot], (size_t)nq * ix->dim_s)) return -1;
        if (l2_reserve(ix->l2_qn[ps.slot], ix->l2_qn_cap[ps.slot], (size_t)nq)) return -1;
        if (l2_reserve(ix->l2_sim[ps.slot], ix->l2_sim_cap[ps.slot], (size_t)nq * k)) return -1;
        if (l2_profile_mark(ix, ps.slot, 0, stream)) return -1;
        HIP_OK(launch_l2_stage_queries(queries, q_dtype, nq, ix->dim, ix->dtype, ix->l2_q[ps.slot], ix->l2_qn[ps.slot], stream));
        if (l2_profile_mark(ix, ps.slot, 1, stream)) return -1;
        ps.queries = ix->l2_q[ps.slot];
        ps.q_dtype = ix->dtype;
        ps.l2_out = out_scores;
        ps.out_scores = ix->l2_sim[ps.slot];
        PendingSearch first = ps;
        first.defer_flags = true;  // the flag words travel behind the finish launch
        if (enqueue_search(ix, first, ix->force_safe != 0, 0, stream)) return -1;
        const SearchWorkspace& ws = ix->ws_lane[ps.lane];
        if (l2_profile_mark(ix, ps.slot, 2, stream) || enqueue_l2_finish(ix, ps, stream) || l2_profile_mark(ix, ps.slot, 3, stream) ||
            hipMemcpyAsync(ix->overflow_host + FLAG_WORDS * ps.slot, ws.overflow, FLAG_WORDS * sizeof(unsigned int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipEventRecord(ix->done[ps.slot], stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(stream);
            return fail("enqueueing the L2 finish failed");
        }
    } else if (ix->exact && nq > 0) {
        // exact mode: the scan fills the slot's top-k' list, the re-scoring kernel behind it writes the caller's rows (no host round
        // trip in between: the list is re-scored even if it later turns out that a candidate list overflowed - finish repeats it then)
        const int kx_formula = exact_kx(ix, k);
        // (adapted to what the last searches of this k needed - finish() - unless the caller fixed the expansion or switched it off)
        const bool adapt = ix->exact_adapt && ix->exact_expand_x100 == 0 && ix->adapt_k == k && ix->adapt_kx >= k;
        const int kx_limit = exact_kx(ix, k, true);
        ps.kx = adapt ? std::min(ix->adapt_kx, kx_limit) : kx_formula;
        if (exact_reserve_lists(ix, ps.slot, (size_t)nq * kx_limit)) return -1;
        PendingSearch in = exact_inner(ix, ps);
        in.defer_flags = true;  // ONE copy of both flag words, behind the re-scoring launch
        if (enqueue_search(ix, in, ix->force_safe != 0, 0, stream)) return -1;
        if (enqueue_exact_list(ix, ps, stream)) {
            (void)hipStreamSynchronize(stream);
            return -1;
        }
    } else if (nq > 0 && enqueue_search(ix, ps, ix->force_safe != 0, 0, stream)) {
        return -1;
    }
    ps.ev_end = ix->ev_used;
    ix->next_slot = (ix->next_slot + 1) % MAX_IN_FLIGHT;
    ix->inflight.push_back(ps);
    return 0;
}

namespace {

// Recovery of a search whose candidate lists overflowed (overflow_host[slot] set): the result is valid (real rows, real scores)
// but may miss hits.  Recovery passes re-scan the store against thresholds seeded from that result - its k-th score is a lower
// bound of the true k-th best, so few rows survive - in 1, 2, 4, ... FILTER stages, and in the exhaustive schedule (dense chunks
// of <= cap rows, cannot overflow) once the stages are that short.  Returns the number of passes run, or -1.
int recover_overflow(vodhip_index* ix, const PendingSearch& ps, hipStream_t stream) {
    PendingSearch rs = ps;  // what the recovery passes search: the whole batch, or only the queries that overflowed
    int pass = 0;
    while (ix->overflow_host[FLAG_WORDS * ps.slot]) {
        if (++pass > 40) return fail("internal error: the exhaustive schedule overflowed");
        ix->last_overflow = 1;
        ix->last_safe_reruns += 1;
        if (pass == 1 && ps.nq <= OVF_ROWS && !ps.band) {
            // the select kernels flagged the queries whose lists overflowed: usually a few (their neighbours are
            // clustered in the store): only they are searched again, as a small batch on the small-batch kernels
            std::vector<unsigned int> flags((size_t)ps.nq);
            HIP_OK(hipMemcpy(flags.data(), ix->ovf_q + (size_t)ps.slot * OVF_ROWS, (size_t)ps.nq * sizeof(unsigned int), hipMemcpyDeviceToHost));
            std::vector<int> rows;
            for (int64_t q = 0; q < ps.nq; ++q)
                if (flags[(size_t)q]) rows.push_back((int)q);
            ix->last_recovered_queries = rows.empty() ? ps.nq : (int64_t)rows.size();
            if (!rows.empty() && (int64_t)rows.size() < ps.nq) {
                int* dmap = ix->q_map + (size_t)ps.slot * OVF_ROWS;
                HIP_OK(hipMemcpy(dmap, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
                rs.q_map = dmap;
                rs.nq = (int64_t)rows.size();
            }
        }
        const size_t ev_first = ix->ev_used;  // behind the events of every younger search in flight
        // (a BAND pass is itself "recovery" pass 1: its overflow passes start at 2 stages)
        if (enqueue_search(ix, rs, false, pass + (ps.band ? 1 : 0), stream)) return -1;
        HIP_OK(hipStreamSynchronize(stream));
        // the recovery launches are accounted separately ("last_recovery_ns"): the time they take is real
        for (size_t e = ev_first; e + 1 < ix->ev_used; e += 2) {
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, ix->ev_pool[e], ix->ev_pool[e + 1]));
            ix->last_recovery_ns += (int64_t)((double)ms * 1e6);
            ++ix->last_recovery_launches;
        }
        ix->ev_used = ev_first;
    }
    return pass;
}

}  // namespace

int vodhip_index_search_finish(vodhip_index_t* ix, void* stream_) {
    if (!ix) return fail("index is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    std::unique_lock<std::mutex> guard(ix->mu);
    if (ix->inflight.empty()) return fail("no search is pending on this index");
    HIP_OK(hipSetDevice(ix->device));
    PendingSearch ps = ix->inflight.front();
    ix->inflight.pop_front();
    if (ps.lane == 1) stream = ix->lane_stream;  // recovery / band passes of a lane-1 search run where the search ran
    if (ps.nq > 0) {
        // this search only: younger ones keep the device busy - and other threads may enqueue more meanwhile (the slot and its
        // event are not reused before MAX_IN_FLIGHT further searches, which cannot be accepted while this one counts as unfinished:
        // `unfinished` below)
        ++ix->unfinished;
        guard.unlock();
        const hipError_t ev_rc = hipEventSynchronize(ix->done[ps.slot]);
        guard.lock();
        --ix->unfinished;
        HIP_OK(ev_rc);
    }
    ix->last_overflow = 0;
    ix->last_safe_reruns = 0;
    ix->last_recovered_queries = 0;
    ix->last_recovery_launches = 0;
    ix->last_recovery_ns = 0;
    ix->last_exact_kx = ps.kx;
    ix->last_exact_band_queries = 0;
    ix->last_exact_band_passes = 0;
    ix->last_exact_need = ps.kx > 0 && ps.nq > 0 ? (int64_t)ix->overflow_host[FLAG_WORDS * ps.slot + 2] : 0;
    ix->last_ring_fallbacks = ps.nq > 0 ? (int64_t)ix->overflow_host[FLAG_WORDS * ps.slot + 3] : 0;  // (before any recovery pass)
    if (ps.kx > 0 && ps.nq > 0 && ix->exact_adapt && ix->exact_expand_x100 == 0) {
        // The list length of the NEXT searches of this k: what this one needed (the list entries within eps of the k-th exact score,
        // maximum over the queries) + 1/16 + 8, rounded up to 8; it rises at once and falls by a quarter of the gap per search.  A list
        // that did not prove complete (need == k') makes the next one a quarter longer, up to the bf16 formula whatever the scan dtype.  A speed knob only: any k' >= k returns
        // the same result (the band pass covers what a short list misses).
        const int need = (int)ix->overflow_host[FLAG_WORDS * ps.slot + 2];
        const int formula = exact_kx(ix, ps.k), limit = exact_kx(ix, ps.k, true);
        // (a list that did not prove complete - need == k' - grows by a quarter, up to the limit; one that did settles at need + 1/16 + 8)
        int target = need >= ps.kx ? std::min(limit, (ps.kx + ps.kx / 4 + 7) / 8 * 8) : std::min(limit, (need + need / 16 + 8 + 7) / 8 * 8);
        target = std::max(target, std::min(formula, ps.k + 8));
        if (ix->adapt_k != ps.k || ix->adapt_kx <= 0) ix->adapt_kx = formula;
        ix->adapt_k = ps.k;
        ix->adapt_kx = target >= ix->adapt_kx ? target : ix->adapt_kx - std::max(8, (ix->adapt_kx - target) / 4 / 8 * 8);
        if (ix->adapt_kx < target) ix->adapt_kx = target;
    }
    if (ps.nq > 0 && ps.kx == 0) {
        const int passes = recover_overflow(ix, ps, stream);
        if (passes < 0) return -1;
        if (passes > 0 && ps.l2_out) {
            // L2 store: the recovery passes seeded from, and rewrote, the similarity-form buffer; the caller's rows are converted
            // from it again, whole (never from the distances the first conversion wrote)
            if (enqueue_l2_finish(ix, ps, stream)) return -1;
            HIP_OK(hipStreamSynchronize(stream));
        }
    } else if (ps.nq > 0) {
        // exact mode.  (1) the scan's own exactness: a recovered list is re-scored again (the first re-scoring saw the incomplete one)
        const int passes = recover_overflow(ix, exact_inner(ix, ps), stream);
        if (passes < 0) return -1;
        if (passes > 0) {
            if (enqueue_exact_list(ix, ps, stream)) return -1;
            HIP_OK(hipStreamSynchronize(stream));
        }
        // (2) the lists that did not prove complete: those queries run a BAND pass (every row whose scan score is within eps of
        // the k-th exact score is re-scored); its own candidate lists may overflow, which splits the pass like any recovery
        if (ix->overflow_host[FLAG_WORDS * ps.slot + 1]) {
            std::vector<unsigned int> flags((size_t)ps.nq);
            HIP_OK(hipMemcpy(flags.data(), ix->x_flag_q + (size_t)ps.slot * OVF_ROWS, (size_t)ps.nq * sizeof(unsigned int), hipMemcpyDeviceToHost));
            std::vector<int> rows;
            for (int64_t q = 0; q < ps.nq; ++q)
                if (flags[(size_t)q]) rows.push_back((int)q);
            ix->last_exact_band_queries = (int64_t)rows.size();
            if (!rows.empty()) {
                PendingSearch bs = ps;
                bs.band = true;
                bs.kx = 0;
                int* dmap = ix->q_map + (size_t)ps.slot * OVF_ROWS;
                if ((int64_t)rows.size() < ps.nq) {
                    HIP_OK(hipMemcpy(dmap, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
                    bs.q_map = dmap;
                    bs.nq = (int64_t)rows.size();
                }
                const size_t ev_first = ix->ev_used;
                if (enqueue_search(ix, bs, false, 1, stream)) return -1;
                HIP_OK(hipStreamSynchronize(stream));
                for (size_t e = ev_first; e + 1 < ix->ev_used; e += 2) {
                    float ms = 0.f;
                    HIP_OK(hipEventElapsedTime(&ms, ix->ev_pool[e], ix->ev_pool[e + 1]));
                    ix->last_recovery_ns += (int64_t)((double)ms * 1e6);
                    ++ix->last_recovery_launches;
                }
                ix->ev_used = ev_first;
                const int more = recover_overflow(ix, bs, stream);
                if (more < 0) return -1;
                ix->last_exact_band_passes = 1 + more;
            }
        }
    }
    ix->last_l2_stage_ns = ix->last_l2_finish_ns = 0;
    if (ps.l2_out && ps.nq > 0 && ix->profile && ix->l2_ev[ps.slot][0] && ix->l2_ev[ps.slot][3]) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, ix->l2_ev[ps.slot][0], ix->l2_ev[ps.slot][1]));
        ix->last_l2_stage_ns = (int64_t)((double)ms * 1e6);
        HIP_OK(hipEventElapsedTime(&ms, ix->l2_ev[ps.slot][2], ix->l2_ev[ps.slot][3]));
        ix->last_l2_finish_ns = (int64_t)((double)ms * 1e6);
    }
    ix->last_filter_launches = (int64_t)((ps.ev_end - ps.ev_begin) / 2);
    ix->last_filter_ns = 0;
    for (size_t e = ps.ev_begin; e + 1 < ps.ev_end; e += 2) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, ix->ev_pool[e], ix->ev_pool[e + 1]));
        ix->last_filter_ns += (int64_t)((double)ms * 1e6);
    }
    return 0;
}

int vodhip_index_search(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, int k, int64_t id_base,
                        float* out_scores, int64_t* out_ids, void* stream) {
    if (vodhip_index_search_async(ix, queries, q_dtype, nq, k, id_base, out_scores, out_ids, stream)) return -1;
    return vodhip_index_search_finish(ix, stream);
}

// ---- listed rows (kernels_listed.hip) -------------------------------------------------------------------------------------
// Nothing here touches the index's search workspace, its FIFO or its query labels: the calls read the store (and the row labels)
// only, so they may run beside searches in flight, on any stream, from several threads.
static int listed_check(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m,
                        const int32_t* q_labels_dev, int n_per_query) {
    if (!ix) return fail("index is NULL");
    if (ix->l2) return fail("listed ids are not supported on an L2 index (VODHIP_L2): score_ids / search_ids need an inner-product store");
    if (m < 1) return fail("m=%lld: a list holds at least one slot", (long long)m);
    if (nq < 0 || (nq > 0 && (!queries || !ids_dev))) return fail("invalid query / id pointers");
    if (q_dtype < 0 || q_dtype > 2) return fail("invalid q_dtype %d", q_dtype);
    if (q_labels_dev && (n_per_query < 1 || n_per_query > 64)) return fail("n_per_query must be in [1, 64]");
    if (q_labels_dev && !ix->row_label) return fail("set the row labels first (vodhip_index_set_row_labels)");
    return 0;
}

static int listed_score(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m,
                        int64_t id_base, const int32_t* q_labels_dev, int n_per_query, float* out, hipStream_t stream) {
    ListedArgs a;
    a.plane = ix->exact ? (const void*)ix->data32 : (const void*)ix->data;
    a.stride = ix->dim_pad;
    a.dim = (int)ix->dim;
    a.dim_pad = (int)ix->dim_pad;
    a.store_dtype = ix->dtype;
    a.exact = ix->exact ? 1 : 0;
    a.q_src = queries;
    a.q_dtype = q_dtype;
    a.ids = ids_dev;
    a.m = m;
    a.id_base = id_base;
    a.ntotal = ix->ntotal;
    a.row_label = ix->row_label;
    a.q_label = q_labels_dev;
    a.n_qlab = q_labels_dev ? n_per_query : 0;
    a.out = out;
    HIP_OK(launch_score_listed(a, nq, stream));
    return 0;
}

int vodhip_index_score_ids(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m,
                           int64_t id_base, const int32_t* q_labels_dev, int n_per_query, float* out_scores, void* stream_) {
    if (listed_check(ix, queries, q_dtype, nq, ids_dev, m, q_labels_dev, n_per_query)) return -1;
    if (nq > 0 && !out_scores) return fail("out_scores is NULL");
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    return listed_score(ix, queries, q_dtype, nq, ids_dev, m, id_base, q_labels_dev, n_per_query, out_scores, (hipStream_t)stream_);
}

int vodhip_index_search_ids(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m, int k,
                            int64_t id_base, const int32_t* q_labels_dev, int n_per_query, float* out_scores, int64_t* out_ids,
                            void* stream_) {
    if (listed_check(ix, queries, q_dtype, nq, ids_dev, m, q_labels_dev, n_per_query)) return -1;
    if (m > VODHIP_MAX_LISTED) return fail("m=%lld exceeds VODHIP_MAX_LISTED=%d for the top-k form", (long long)m, VODHIP_MAX_LISTED);
    if (k < 1 || k > VODHIP_MAX_K) return fail("k=%d out of range [1, %d]", k, VODHIP_MAX_K);
    if (nq > 0 && (!out_scores || !out_ids)) return fail("invalid output pointers");
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    float* aligned = nullptr;  // stream-ordered temporary: the aligned scores the select reads
    HIP_OK(hipMallocAsync((void**)&aligned, (size_t)nq * (size_t)m * sizeof(float), stream));
    int rc = listed_score(ix, queries, q_dtype, nq, ids_dev, m, id_base, q_labels_dev, n_per_query, aligned, stream);
    if (!rc) {
        const hipError_t e = launch_select_listed(aligned, ids_dev, nq, m, k, id_base, out_scores, out_ids, stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rc = fail("select of the listed scores failed: %s", hipGetErrorString(e));
        }
    }
    const std::string keep = rc ? g_last_error : std::string();
    const hipError_t fe = hipFreeAsync(aligned, stream);
    if (rc) return fail("%s", keep.c_str());
    HIP_OK(fe);
    return 0;
}

// the weighted sum of listed rows (H2w): the partials of lists longer than one chunk are a stream-ordered temporary of at most
// VODHIP_SUM_IDS_TEMP_BYTES (or one query's), filled and folded a slice of the batch at a time - a query's bits do not depend on the slice
int vodhip_index_sum_ids(vodhip_index_t* ix, const int64_t* ids_dev, const float* weights_dev, int64_t nq, int64_t m, int64_t id_base,
                         const int32_t* q_labels_dev, int n_per_query, float* out, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (ix->l2) return fail("listed ids are not supported on an L2 index (VODHIP_L2): sum_ids needs an inner-product store");
    if (m < 1) return fail("m=%lld: a list holds at least one slot", (long long)m);
    if (nq < 0 || (nq > 0 && (!ids_dev || !weights_dev || !out))) return fail("invalid id / weight / output pointers");
    if (q_labels_dev && (n_per_query < 1 || n_per_query > 64)) return fail("n_per_query must be in [1, 64]");
    if (q_labels_dev && !ix->row_label) return fail("set the row labels first (vodhip_index_set_row_labels)");
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    ListedArgs a;
    a.plane = ix->exact ? (const void*)ix->data32 : (const void*)ix->data;
    a.stride = ix->dim_pad;
    a.dim = (int)ix->dim;
    a.dim_pad = (int)ix->dim_pad;
    a.store_dtype = ix->dtype;
    a.exact = ix->exact ? 1 : 0;
    a.m = m;
    a.id_base = id_base;
    a.ntotal = ix->ntotal;
    a.row_label = ix->row_label;
    a.n_qlab = q_labels_dev ? n_per_query : 0;
    const int64_t chunks = listed_sum_chunks(m);
    const size_t per_query = (size_t)chunks * (size_t)ix->dim * sizeof(float);
    const int64_t slice = chunks == 1 ? nq : std::min<int64_t>(nq, std::max<int64_t>(1, (int64_t)((size_t)VODHIP_SUM_IDS_TEMP_BYTES / per_query)));
    if (chunks > 1) {
        if (hipError_t e = hipMallocAsync((void**)&a.part, per_query * (size_t)slice, stream); e != hipSuccess) {
            (void)hipGetLastError();
            return fail("hipMallocAsync of the %zu-byte partial sums failed: %s", per_query * (size_t)slice, hipGetErrorString(e));
        }
    }
    hipError_t le = hipSuccess;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) {
        a.ids = ids_dev + q0 * m;
        a.weights = weights_dev + q0 * m;
        a.q_label = q_labels_dev ? q_labels_dev + q0 * n_per_query : nullptr;
        a.out = out + q0 * ix->dim;
        le = launch_sum_listed(a, std::min(slice, nq - q0), stream);
    }
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = a.part ? hipFreeAsync(a.part, stream) : hipSuccess;
    if (le != hipSuccess) return fail("launch of the listed-row sum failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

// ---- the whole-store scans (store_scan.h): log_partition, posterior_stats, posterior_divergence, the rank calls, posterior_mean, sample_posterior ----------
// Like the listed calls they read the store (and the row labels) only.  What the flat calls share:

// a message of log_partition_args_error, as the flat calls report it
static int partition_args_fail(const char* msg, int q_dtype, float beta) {
    if (!strcmp(msg, "invalid q_dtype")) return fail("invalid q_dtype %d", q_dtype);
    if (!strncmp(msg, "beta", 4)) return fail("beta=%g: %s", (double)beta, msg);
    return fail("%s", msg);
}

// the indexes no scan accepts; `what` names the operation in the message
static int scan_refusal(const vodhip_index_t* ix, const char* what, const void* q_labels_dev) {
    if (ix->l2) return fail(SCAN_REFUSES_L2, what);
    if (ix->exact) return fail(SCAN_REFUSES_EXACT_F32, what);
    if (q_labels_dev && !ix->row_label) return fail("set the row labels first (vodhip_index_set_row_labels)");
    return 0;
}

static void fill_scan_inputs(ScanInputs& s, const vodhip_index_t* ix, const void* queries, int q_dtype, const int32_t* q_labels_dev, int n_per_query) {
    s.store = ix->data;
    s.dim = ix->dim;
    s.dim_pad = ix->dim_pad;
    s.ntotal = ix->ntotal;
    s.store_dtype = ix->dtype;
    s.q_src = queries;
    s.q_dtype = q_dtype;
    s.row_label = ix->row_label;
    s.q_label = q_labels_dev;
    s.n_qlab = q_labels_dev ? n_per_query : 0;
}

// queries (or pairs) per slice of a batch under the index's budget (scan_slices.h), remembered for "last_scan_slice" /
// "last_scan_per_query_bytes"
static int64_t index_scan_slice(vodhip_index_t* ix, size_t per_query) {
    const int64_t slice = scan_slice_queries(ix->scan_temp_bytes, per_query);
    ix->last_scan[0] = slice;
    ix->last_scan[1] = (int64_t)per_query;
    return slice;
}

// the stream-ordered temporaries of a call: one block per byte count, none (NULL) for a count of 0
struct ScanTemps {
    static constexpr int MAX = 4;
    void* p[MAX] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t stream = nullptr;
    int alloc(std::initializer_list<size_t> bytes) {  // 0, or the failure reported with nothing left allocated
        int i = 0;
        for (const size_t n : bytes) {
            if (n != 0) {
                if (hipError_t e = hipMallocAsync(&p[i], n, stream); e != hipSuccess) {
                    (void)hipGetLastError();
                    p[i] = nullptr;
                    (void)release();
                    return fail("hipMallocAsync of a %zu-byte temporary failed: %s", n, hipGetErrorString(e));
                }
            }
            ++i;
        }
        return 0;
    }
    hipError_t release() {  // frees every block behind the launches; the first error
        hipError_t fe = hipSuccess;
        for (void*& q : p) {
            if (q)
                if (hipError_t e = hipFreeAsync(q, stream); e != hipSuccess && fe == hipSuccess) fe = e;
            q = nullptr;
        }
        return fe;
    }
};

// ---- log-partition scan (kernels_partition.hip): staged queries and partials are stream-ordered temporaries ----------------------
int vodhip_index_log_partition(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev,
                               int n_per_query, float* out_max, float* out_log_rel, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = log_partition_args_error(queries, q_dtype, nq, beta, q_labels_dev, n_per_query, out_max, out_log_rel))
        return partition_args_fail(msg, q_dtype, beta);
    if (scan_refusal(ix, "log_partition", q_labels_dev)) return -1;
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    constexpr int64_t Q_CHUNK = 1024;  // queries per scan launch (a multiple of the query tile): bounds the partials' size
    PartitionArgs a;
    fill_scan_inputs(a, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.beta = beta;
    a.out_max = out_max;
    a.out_log_rel = out_log_rel;
    const int64_t nq_pad = scan_nq_pad(std::min(nq, Q_CHUNK));
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * (size_t)ix->dim_pad * 2, std::max<size_t>(8, (size_t)scan_tiles(a.ntotal) * (size_t)nq_pad * 8)})) return -1;
    a.q_stage = tmp.p[0];
    a.part = tmp.p[1];
    hipError_t le = hipSuccess;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += Q_CHUNK) le = launch_log_partition(a, q0, std::min(Q_CHUNK, nq - q0), stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    if (le != hipSuccess) return fail("log-partition launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

// ---- posterior statistics (kernels_stats.hip): the log-partition scan with two more accumulators; 16-byte partials, so the batch runs
// in slices that keep them under VODHIP_POSTERIOR_TEMP_BYTES ------------------------------------------------------------------------
int vodhip_index_posterior_stats(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev,
                                 int n_per_query, float* out_max, float* out_log_rel, float* out_mean_rel, float* out_var, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = posterior_stats_args_error(queries, q_dtype, nq, beta, q_labels_dev, n_per_query, out_max, out_log_rel, out_mean_rel, out_var))
        return partition_args_fail(msg, q_dtype, beta);
    if (scan_refusal(ix, "posterior_stats", q_labels_dev)) return -1;
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    StatsArgs a;
    fill_scan_inputs(a, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.beta = beta;
    a.out_max = out_max;
    a.out_log_rel = out_log_rel;
    a.out_mean_rel = out_mean_rel;
    a.out_var = out_var;
    const size_t per_query = std::max<size_t>(1, (size_t)scan_tiles(a.ntotal)) * 16;  // the partials
    const int64_t slice = index_scan_slice(ix, per_query);
    const int64_t nq_pad = scan_nq_pad(std::min(nq, slice));
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * (size_t)ix->dim_pad * 2, per_query * (size_t)nq_pad})) return -1;
    a.q_stage = tmp.p[0];
    a.part = tmp.p[1];
    hipError_t le = hipSuccess;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) le = launch_posterior_stats(a, q0, std::min(slice, nq - q0), stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    if (le != hipSuccess) return fail("posterior-stats launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

// ---- posterior divergence (kernels_divergence.hip): the posterior-stats scan over the two staged queries of every pair; 32 bytes of
// partials per (pair, tile), sliced as above ------------------------------------------------------------------------------------------
int vodhip_index_posterior_divergence(vodhip_index_t* ix, const void* queries_a, const void* queries_b, int q_dtype, int64_t nq, float beta_a,
                                      float beta_b, const int32_t* q_labels_dev, int n_per_query, float* out_max_a, float* out_log_rel_a,
                                      float* out_mean_rel_a, float* out_cross_rel_ab, float* out_max_b, float* out_log_rel_b,
                                      float* out_mean_rel_b, float* out_cross_rel_ba, void* stream_) {
    if (!ix) return fail("index is NULL");
    float* const outs[8] = {out_max_a, out_log_rel_a, out_mean_rel_a, out_cross_rel_ab, out_max_b, out_log_rel_b, out_mean_rel_b, out_cross_rel_ba};
    if (const char* msg = posterior_divergence_args_error(queries_a, queries_b, q_dtype, nq, beta_a, beta_b, q_labels_dev, n_per_query, (const void* const*)outs)) {
        if (!strcmp(msg, "invalid q_dtype")) return fail("invalid q_dtype %d", q_dtype);
        if (!strncmp(msg, "beta_a", 6)) return fail("beta_a=%g: %s", (double)beta_a, msg);
        if (!strncmp(msg, "beta_b", 6)) return fail("beta_b=%g: %s", (double)beta_b, msg);
        return fail("%s", msg);
    }
    if (scan_refusal(ix, "posterior_divergence", q_labels_dev)) return -1;
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    DivergenceArgs a;
    fill_scan_inputs(a, ix, queries_a, q_dtype, q_labels_dev, n_per_query);
    a.q_src_b = queries_b;
    a.beta_a = beta_a;
    a.beta_b = beta_b;
    for (int k = 0; k < 8; ++k) a.out[k] = outs[k];
    const size_t per_pair = std::max<size_t>(1, (size_t)scan_tiles(a.ntotal)) * 32;  // the partials
    const int64_t slice = index_scan_slice(ix, per_pair);                             // pairs of a launch
    const int64_t nq_pad = scan_nq_pad(2 * std::min(nq, slice));                     // staged queries of a launch
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * (size_t)ix->dim_pad * 2, per_pair * (size_t)(nq_pad / 2)})) return -1;
    a.q_stage = tmp.p[0];
    a.part = tmp.p[1];
    hipError_t le = hipSuccess;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) le = launch_posterior_divergence(a, q0, std::min(slice, nq - q0), stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    if (le != hipSuccess) return fail("posterior-divergence launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

// ---- exact ranks (kernels_rank.hip): pick the listed pairs' scan scores, count the store against them -----------------------------
static int rank_call(vodhip_index_t* ix, int mode, const char* what, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev,
                     const float* thresholds_dev, const int64_t* tie_ids_dev, int64_t m, int64_t id_base, const int32_t* q_labels_dev,
                     int n_per_query, int64_t* out_counts, float* out_scores, int32_t* out_rows, hipStream_t stream) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = rank_args_error(queries, q_dtype, nq, m, q_labels_dev, n_per_query)) {
        if (!strcmp(msg, "invalid q_dtype")) return fail("invalid q_dtype %d", q_dtype);
        if (msg[0] == 'm') return fail("m=%lld: %s", (long long)m, msg + 2);
        return fail("%s", msg);
    }
    if (nq > 0) {
        if (mode != RANK_MODE_THRESHOLDS && !ids_dev) return fail("ids is NULL");
        if (mode == RANK_MODE_THRESHOLDS && !thresholds_dev) return fail("thresholds is NULL");
        if (mode != RANK_MODE_PICK && !out_counts) return fail(mode == RANK_MODE_RANK ? "out_ranks is NULL" : "out_counts is NULL");
        if (mode != RANK_MODE_THRESHOLDS && !out_scores) return fail("out_scores is NULL");
    }
    if (scan_refusal(ix, what, q_labels_dev)) return -1;
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    RankArgs a;
    fill_scan_inputs(a, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.m = m;
    a.id_base = id_base;
    a.ids = ids_dev;
    a.thresholds = thresholds_dev;
    a.tie_ids = tie_ids_dev;
    a.out_score = out_scores;
    a.out_rows = out_rows;
    a.out_count = out_counts;
    const bool pick = mode != RANK_MODE_THRESHOLDS, count = mode != RANK_MODE_PICK;
    // a query's gathered rows are at most m + 3 rows of the mini-store
    const size_t row_bytes = (size_t)ix->dim_pad * 2;
    const int64_t slice = index_scan_slice(ix, row_bytes * (size_t)(1 + (pick ? m + 3 : 0)) + (size_t)m * 16);
    const int64_t nq_pad = scan_nq_pad(std::min(nq, slice));
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * row_bytes, pick ? (size_t)rank_mini_rows(nq_pad, m) * row_bytes : 0, pick ? (size_t)nq_pad * (size_t)m * 4 : 0,
                   count ? (size_t)nq_pad * (size_t)m * 12 : 0}))
        return -1;
    a.q_stage = tmp.p[0];
    a.mini = tmp.p[1];
    a.slot_row = (int*)tmp.p[2];
    a.table = (unsigned int*)tmp.p[3];
    hipError_t le = hipSuccess;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) le = launch_rank(a, mode, q0, std::min(slice, nq - q0), stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    if (le != hipSuccess) return fail("%s launch failed: %s", what, hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

int vodhip_index_count_above(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, const float* thresholds_dev,
                             const int64_t* tie_ids_dev, int64_t m, int64_t id_base, const int32_t* q_labels_dev, int n_per_query,
                             int64_t* out_counts, void* stream_) {
    return rank_call(ix, RANK_MODE_THRESHOLDS, "count_above", queries, q_dtype, nq, nullptr, thresholds_dev, tie_ids_dev, m, id_base, q_labels_dev,
                     n_per_query, out_counts, nullptr, nullptr, (hipStream_t)stream_);
}

int vodhip_index_rank_ids(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m, int64_t id_base,
                          const int32_t* q_labels_dev, int n_per_query, int64_t* out_ranks, float* out_scores, void* stream_) {
    return rank_call(ix, RANK_MODE_RANK, "rank_ids", queries, q_dtype, nq, ids_dev, nullptr, nullptr, m, id_base, q_labels_dev, n_per_query, out_ranks,
                     out_scores, nullptr, (hipStream_t)stream_);
}

int vodhip_index_scan_score_ids(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, const int64_t* ids_dev, int64_t m,
                                int64_t id_base, const int32_t* q_labels_dev, int n_per_query, float* out_scores, int32_t* out_rows,
                                void* stream_) {
    return rank_call(ix, RANK_MODE_PICK, "scan_score_ids", queries, q_dtype, nq, ids_dev, nullptr, nullptr, m, id_base, q_labels_dev, n_per_query,
                     nullptr, out_scores, out_rows, (hipStream_t)stream_);
}

// ---- range scan (kernels_range.hip): count pass, prefix, lims and - with outputs - the emit pass, slice by slice ------------------
int vodhip_index_range_search(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, const float* thresholds_dev,
                              const int64_t* tie_ids_dev, int64_t id_base, const int32_t* q_labels_dev, int n_per_query, int64_t* lims_dev,
                              float* out_scores_dev, int64_t* out_ids_dev, int64_t capacity, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = range_args_error(queries, q_dtype, nq, thresholds_dev, q_labels_dev, n_per_query, lims_dev, out_scores_dev, out_ids_dev, capacity)) {
        if (!strcmp(msg, "invalid q_dtype")) return fail("invalid q_dtype %d", q_dtype);
        if (!strncmp(msg, "capacity", 8)) return fail("capacity=%lld: %s", (long long)capacity, msg);
        return fail("%s", msg);
    }
    if (scan_refusal(ix, "range_search", q_labels_dev)) return -1;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    const bool emit = out_scores_dev != nullptr;
    for (auto& w : ix->last_range) w = 0;
    if (nq == 0) {
        HIP_OK(hipMemsetAsync(lims_dev, 0, sizeof(int64_t), stream));
        return 0;
    }
    RangeArgs a;
    fill_scan_inputs(a, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.id_base = id_base;
    a.thresholds = thresholds_dev;
    a.tie_ids = tie_ids_dev;
    a.lims = lims_dev;
    a.out_scores = out_scores_dev;
    a.out_ids = out_ids_dev;
    a.capacity = capacity;
    const size_t row_bytes = (size_t)ix->dim_pad * 2;
    const size_t n_tiles = (size_t)scan_tiles(a.ntotal);
    const int64_t slice = index_scan_slice(ix, std::max<size_t>(1, n_tiles) * 4 + row_bytes + 12);  // the count table, the staged query, the words
    const int64_t nq_pad = scan_nq_pad(std::min(nq, slice));
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * row_bytes, n_tiles * (size_t)nq_pad * 4, (size_t)nq_pad * 12, emit ? RGS_WORDS * sizeof(unsigned int) : 0})) return -1;
    a.q_stage = tmp.p[0];
    a.table = (int*)tmp.p[1];
    a.words = (unsigned int*)tmp.p[2];
    a.status = (unsigned int*)tmp.p[3];
    hipError_t le = emit ? hipMemsetAsync(a.status, 0, RGS_WORDS * sizeof(unsigned int), stream) : hipSuccess;
    int64_t emit_groups = 0;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) {
        const int64_t n = std::min(slice, nq - q0);
        le = launch_range(a, q0, n, stream);
        emit_groups += (int64_t)n_tiles * (scan_nq_pad(n) / (n <= 64 ? 64 : 128));
    }
    // With outputs the call reports an overflow itself: the status words and lims[nq] come back, which waits for the stream
    unsigned int st[RGS_WORDS] = {};
    int64_t total = 0;
    if (emit && le == hipSuccess) le = hipMemcpyAsync(st, a.status, sizeof(st), hipMemcpyDeviceToHost, stream);
    if (emit && le == hipSuccess) le = hipMemcpyAsync(&total, lims_dev + nq, sizeof(total), hipMemcpyDeviceToHost, stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    const hipError_t se = emit ? hipStreamSynchronize(stream) : hipSuccess;
    if (le != hipSuccess) return fail("range_search launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    HIP_OK(se);
    if (emit) {
        ix->last_range[0] = total > capacity ? total - capacity : 0;
        ix->last_range[1] = st[RGS_SELFCHECK];
        ix->last_range[2] = st[RGS_SKIPPED];
        ix->last_range[3] = emit_groups;
        if (total > capacity)
            return fail("range_search: the result holds %lld rows, the outputs %lld (capacity); lims is complete, rows at positions below the capacity are written",
                        (long long)total, (long long)capacity);
    }
    return 0;
}

// ---- posterior mean (kernels_posterior.hip): the log-partition launches, then the second scan and its finish -------------------
int vodhip_index_posterior_mean(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev,
                                int n_per_query, float* out_max, float* out_log_rel, float* out_mean, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = log_partition_args_error(queries, q_dtype, nq, beta, q_labels_dev, n_per_query, out_max, out_log_rel))
        return partition_args_fail(msg, q_dtype, beta);
    if (nq > 0 && !out_mean) return fail("invalid query / output pointers");
    if (scan_refusal(ix, "log_partition", q_labels_dev)) return -1;  // (the name these two refusals have always carried here)
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    PosteriorArgs a;
    fill_scan_inputs(a.p, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.p.beta = beta;
    a.p.out_max = out_max;
    a.p.out_log_rel = out_log_rel;
    a.out_mean = out_mean;
    const size_t per_query = std::max<size_t>(1, (size_t)posterior_mean_groups(a.p.ntotal)) * (size_t)ix->dim_pad * sizeof(float);  // the group accumulators
    const int64_t slice = index_scan_slice(ix, per_query);
    const int64_t nq_pad = scan_nq_pad(std::min(nq, slice));
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * (size_t)ix->dim_pad * 2, std::max<size_t>(8, (size_t)scan_tiles(a.p.ntotal) * (size_t)nq_pad * 8), per_query * (size_t)nq_pad}))
        return -1;
    a.p.q_stage = tmp.p[0];
    a.p.part = tmp.p[1];
    a.acc = (float*)tmp.p[2];
    hipError_t le = hipSuccess;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) le = launch_posterior_mean(a, q0, std::min(slice, nq - q0), stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    if (le != hipSuccess) return fail("posterior-mean launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

// ---- posterior read-out (kernels_readout.hip): ONE scan - partition partials, running-maximum value accumulators - and two finishes ----
int vodhip_index_posterior_expectation(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev,
                                       int n_per_query, float* out_max, float* out_log_rel, float* out_values, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = posterior_expectation_args_error(queries, q_dtype, nq, beta, q_labels_dev, n_per_query, out_max, out_log_rel, out_values))
        return partition_args_fail(msg, q_dtype, beta);
    if (scan_refusal(ix, "posterior_expectation", q_labels_dev)) return -1;
    if (!ix->row_value) return fail("posterior_expectation: the index has no value table (vodhip_index_set_row_values)");
    if (ix->value_rows != ix->ntotal)
        return fail("posterior_expectation: the value table holds %lld rows, the index %lld: set the table again after adding rows", (long long)ix->value_rows,
                    (long long)ix->ntotal);
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    ReadoutArgs a;
    fill_scan_inputs(a.p, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.p.beta = beta;
    a.p.out_max = out_max;
    a.p.out_log_rel = out_log_rel;
    a.values = ix->row_value;
    a.n_cols = (int)ix->value_cols;
    a.c_pad = (int)ix->value_c_pad;
    a.out_values = out_values;
    const size_t acc_per_query = std::max<size_t>(1, (size_t)readout_groups(a.p.ntotal)) * (size_t)a.c_pad * sizeof(float);  // the group accumulators
    const size_t part_per_query = std::max<size_t>(1, (size_t)scan_tiles(a.p.ntotal)) * 8;                                 // the partition partials
    const int64_t slice = index_scan_slice(ix, acc_per_query + part_per_query);
    const int64_t nq_pad = scan_nq_pad(std::min(nq, slice));
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * (size_t)ix->dim_pad * 2, part_per_query * (size_t)nq_pad, acc_per_query * (size_t)nq_pad})) return -1;
    a.p.q_stage = tmp.p[0];
    a.p.part = tmp.p[1];
    a.acc = (float*)tmp.p[2];
    hipError_t le = hipSuccess;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) le = launch_posterior_expectation(a, q0, std::min(slice, nq - q0), stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    if (le != hipSuccess) return fail("posterior-expectation launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

// the column maxima of the value table: once per table; the first call waits for them, so that a later call on any stream may read them
static int ensure_value_vmax(vodhip_index_t* ix, const char* what, hipStream_t stream) {
    std::lock_guard<std::mutex> guard(ix->mu);
    if (ix->value_vmax_ready) return 0;
    if (!ix->value_vmax) HIP_OK(hipMalloc((void**)&ix->value_vmax, (size_t)ix->value_c_pad * sizeof(float)));
    const hipError_t e = launch_readout_grad_vmax(ix->row_value, ix->value_rows, (int)ix->value_c_pad, ix->dtype, ix->value_vmax, stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail("%s launch failed: %s", what, hipGetErrorString(e));
    }
    HIP_OK(hipStreamSynchronize(stream));
    ix->value_vmax_ready = true;
    return 0;
}

// ---- the read-out's gradient in the query (kernels_readout_grad.hip): g staged, ONE scan behind the forward's words, one finish ----
int vodhip_index_posterior_expectation_backward(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev,
                                                int n_per_query, const float* max_score, const float* log_rel, const float* values, const float* grad_values,
                                                float* out_grad_queries, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = posterior_expectation_backward_args_error(queries, q_dtype, nq, beta, q_labels_dev, n_per_query, max_score, log_rel, values, grad_values,
                                                                    out_grad_queries))
        return partition_args_fail(msg, q_dtype, beta);
    if (scan_refusal(ix, "posterior_expectation_backward", q_labels_dev)) return -1;
    if (!ix->row_value) return fail("posterior_expectation_backward: the index has no value table (vodhip_index_set_row_values)");
    if (ix->value_rows != ix->ntotal)
        return fail("posterior_expectation_backward: the value table holds %lld rows, the index %lld: set the table again after adding rows",
                    (long long)ix->value_rows, (long long)ix->ntotal);
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    if (ensure_value_vmax(ix, "posterior-expectation-backward", stream)) return -1;
    ReadoutGradArgs a;
    fill_scan_inputs(a.p, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.p.beta = beta;
    a.p.out_max = const_cast<float*>(max_score);  // (read only: ReadoutGradArgs)
    a.p.out_log_rel = const_cast<float*>(log_rel);
    a.values = ix->row_value;
    a.n_cols = (int)ix->value_cols;
    a.c_pad = (int)ix->value_c_pad;
    a.vmax = ix->value_vmax;
    a.y = values;
    a.g = grad_values;
    a.out_grad = out_grad_queries;
    const size_t groups = std::max<size_t>(1, (size_t)readout_groups(a.p.ntotal));
    const size_t acc_per_query = groups * (size_t)ix->dim_pad * sizeof(float);  // the group accumulators
    const size_t mg_per_query = groups * sizeof(float);                          // the group maxima
    const size_t small_per_query = (size_t)a.c_pad * 2 + readout_grad_aux_bytes();
    const int64_t slice = index_scan_slice(ix, acc_per_query + mg_per_query + small_per_query);
    const int64_t nq_pad = scan_nq_pad(std::min(nq, slice));
    ScanTemps tmp, tmp2;
    tmp.stream = tmp2.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * (size_t)ix->dim_pad * 2, acc_per_query * (size_t)nq_pad, mg_per_query * (size_t)nq_pad, (size_t)nq_pad * (size_t)a.c_pad * 2})) return -1;
    if (tmp2.alloc({(size_t)nq_pad * readout_grad_aux_bytes()})) {
        (void)tmp.release();
        return -1;
    }
    a.p.q_stage = tmp.p[0];
    a.acc = (float*)tmp.p[1];
    a.mg = (float*)tmp.p[2];
    a.g_stage = tmp.p[3];
    a.aux = tmp2.p[0];
    hipError_t le = hipSuccess;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) le = launch_posterior_expectation_backward(a, q0, std::min(slice, nq - q0), stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    const hipError_t fe2 = tmp2.release();
    if (le != hipSuccess) return fail("posterior-expectation-backward launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    HIP_OK(fe2);
    return 0;
}

// ---- the read-out's adjoint, its gradient in the table (kernels_readout_adjoint.hip): the column exponents, then per slice of 1024 queries
// the two stagings and ONE scan whose workgroups own their output rows ----
int vodhip_index_posterior_adjoint(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev, int n_per_query,
                                   const float* max_score, const float* log_rel, const float* weights, int64_t n_cols, int accumulate, float* out, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = posterior_adjoint_args_error(queries, q_dtype, nq, beta, q_labels_dev, n_per_query, max_score, log_rel, weights, n_cols, out))
        return partition_args_fail(msg, q_dtype, beta);
    if (scan_refusal(ix, "posterior_adjoint", q_labels_dev)) return -1;
    if (ix->ntotal == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    if (nq == 0) {
        if (!accumulate) HIP_OK(hipMemsetAsync(out, 0, (size_t)ix->ntotal * (size_t)n_cols * sizeof(float), stream));
        return 0;
    }
    ReadoutAdjointArgs a;
    fill_scan_inputs(a.p, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.p.beta = beta;
    a.p.out_max = const_cast<float*>(max_score);  // (read only: ReadoutAdjointArgs)
    a.p.out_log_rel = const_cast<float*>(log_rel);
    a.w = weights;
    a.n_cols = (int)n_cols;
    a.c_pad = (int)readout_adjoint_c_pad(n_cols);
    a.out = out;
    const int64_t slice = READOUT_ADJOINT_SLICE;
    const int64_t nq_pad = readout_adjoint_nq_pad(std::min(nq, slice));
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * (size_t)ix->dim_pad * 2, (size_t)nq_pad * (size_t)a.c_pad * 2, (size_t)a.c_pad * sizeof(int)})) return -1;
    a.p.q_stage = tmp.p[0];
    a.w_stage = tmp.p[1];
    a.col_k = tmp.p[2];
    hipError_t le = launch_readout_adjoint_columns(a, nq, stream);
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice)
        le = launch_posterior_adjoint(a, q0, std::min(slice, nq - q0), (q0 > 0 || accumulate) ? 1 : 0, stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    if (le != hipSuccess) return fail("posterior-adjoint launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

// ---- the posterior's gradient in the stored rows (kernels_key_grad.hip): the batch-wide scales, then per slice of 1024 queries the
// stagings and ONE scan whose workgroups own their output rows.  vmax_dev: the column maxima the scales are formed from - NULL = the
// index's own (the flat call); a node index hands every shard the maxima over all the rows (vodhip_node.hip) ----
static int index_key_gradient(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev, int n_per_query,
                              const float* max_score, const float* log_rel, const float* grad_log_z, const float* values, const float* grad_values,
                              const float* vmax_dev, int accumulate, float* out, hipStream_t stream) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = posterior_key_gradient_args_error(queries, q_dtype, nq, beta, q_labels_dev, n_per_query, max_score, log_rel, grad_log_z, values,
                                                            grad_values, out))
        return partition_args_fail(msg, q_dtype, beta);
    if (scan_refusal(ix, "posterior_key_gradient", q_labels_dev)) return -1;
    if (grad_values) {
        if (!ix->row_value) return fail("posterior_key_gradient: grad_values needs a value table (vodhip_index_set_row_values)");
        if (ix->value_rows != ix->ntotal)
            return fail("posterior_key_gradient: the value table holds %lld rows, the index %lld: set the table again after adding rows", (long long)ix->value_rows,
                        (long long)ix->ntotal);
    }
    if (ix->ntotal == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    if (nq == 0) {
        if (!accumulate) HIP_OK(hipMemsetAsync(out, 0, (size_t)ix->ntotal * (size_t)ix->dim * sizeof(float), stream));
        return 0;
    }
    if (nq > 0x7fffffffll) return fail("posterior_key_gradient: nq=%lld is beyond 2^31 - 1", (long long)nq);
    if (grad_values && !vmax_dev && ensure_value_vmax(ix, "posterior-key-gradient", stream)) return -1;
    KeyGradArgs a;
    fill_scan_inputs(a.p, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.p.beta = beta;
    a.p.out_max = const_cast<float*>(max_score);  // (read only: KeyGradArgs)
    a.p.out_log_rel = const_cast<float*>(log_rel);
    a.a = grad_log_z;
    a.g = grad_values;
    if (grad_values) {
        a.y = values;
        a.values = ix->row_value;
        a.n_cols = (int)ix->value_cols;
        a.c_pad = (int)ix->value_c_pad;
        a.vmax = vmax_dev ? vmax_dev : ix->value_vmax;
    }
    a.out = out;
    const int64_t slice = KEY_GRAD_SLICE;
    const int64_t nq_pad = key_grad_nq_pad(std::min(nq, slice));
    ScanTemps tmp;
    tmp.stream = stream;
    if (tmp.alloc({(size_t)nq_pad * (size_t)ix->dim_pad * 2, (size_t)nq_pad * (size_t)a.c_pad * 2, (size_t)nq * key_grad_aux_bytes(), key_grad_scales_bytes()})) return -1;
    a.p.q_stage = tmp.p[0];
    a.g_stage = tmp.p[1];
    a.aux = tmp.p[2];
    a.scales = tmp.p[3];
    hipError_t le = launch_key_grad_scales(a, nq, stream);
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice)
        le = launch_posterior_key_gradient(a, q0, std::min(slice, nq - q0), (q0 > 0 || accumulate) ? 1 : 0, stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t fe = tmp.release();
    if (le != hipSuccess) return fail("posterior-key-gradient launch failed: %s", hipGetErrorString(le));
    HIP_OK(fe);
    return 0;
}

int vodhip_index_posterior_key_gradient(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev, int n_per_query,
                                        const float* max_score, const float* log_rel, const float* grad_log_z, const float* values, const float* grad_values,
                                        int accumulate, float* out, void* stream_) {
    return index_key_gradient(ix, queries, q_dtype, nq, beta, q_labels_dev, n_per_query, max_score, log_rel, grad_log_z, values, grad_values, nullptr, accumulate, out,
                              (hipStream_t)stream_);
}

// ---- posterior sampling (kernels_sample_posterior.hip): the log-partition launches, key-max scan, threshold, emit scan, select ------
int vodhip_index_sample_posterior(vodhip_index_t* ix, const void* queries, int q_dtype, int64_t nq, int k, float beta, uint64_t seed,
                                  int64_t query_offset, int64_t id_base, const int32_t* q_labels_dev, int n_per_query, float* out_max,
                                  float* out_log_rel, int64_t* out_ids, float* out_scores, float* out_log_p, float* out_log_weight,
                                  float* out_keys, void* stream_) {
    if (!ix) return fail("index is NULL");
    if (const char* msg = log_partition_args_error(queries, q_dtype, nq, beta, q_labels_dev, n_per_query, out_max, out_log_rel))
        return partition_args_fail(msg, q_dtype, beta);
    if (const char* msg = sample_posterior_args_error(nq, k, query_offset, id_base, out_ids, out_scores, out_log_p, out_log_weight, out_keys)) {
        if (msg[0] == 'k') return fail("k=%d: %s", k, msg);
        return fail("%s", msg);
    }
    if (scan_refusal(ix, "sample_posterior", q_labels_dev)) return -1;
    if (nq == 0) return 0;
    HIP_OK(hipSetDevice(ix->device));
    hipStream_t stream = (hipStream_t)stream_;
    PosteriorSampleArgs a;
    fill_scan_inputs(a.p, ix, queries, q_dtype, q_labels_dev, n_per_query);
    a.p.beta = beta;
    a.p.out_max = out_max;
    a.p.out_log_rel = out_log_rel;
    a.k = k;
    a.seed = seed;
    a.query_offset = query_offset;
    a.id_base = id_base;
    a.stride = sample_posterior_stride(a.p.ntotal, k);
    a.out_ids = out_ids;
    a.out_scores = out_scores;
    a.out_log_p = out_log_p;
    a.out_log_weight = out_log_weight;
    a.out_keys = out_keys;
    const size_t n_tiles = std::max<size_t>(1, (size_t)scan_tiles(a.p.ntotal));
    const int64_t slice = index_scan_slice(ix, (size_t)a.stride * 12 + n_tiles * 12);  // the candidate lists and the tile words
    const int64_t nq_pad = scan_nq_pad(std::min(nq, slice));
    constexpr int NT = 7;
    const size_t bytes[NT] = {(size_t)nq_pad * (size_t)ix->dim_pad * 2, n_tiles * (size_t)nq_pad * 8, n_tiles * (size_t)nq_pad * 4,
                              (size_t)nq_pad * (size_t)a.stride * 8, (size_t)nq_pad * (size_t)a.stride * 4,
                              (size_t)sample_posterior_ctl_words(nq_pad) * 4, 8 * sizeof(unsigned int)};
    size_t off[NT + 1] = {0};
    for (int i = 0; i < NT; ++i) off[i + 1] = off[i] + (bytes[i] + 255) / 256 * 256;
    std::lock_guard<std::mutex> guard(ix->sample_mu);
    if (ix->sample_ws_bytes < off[NT]) {  // (the previous call has waited for its stream: nothing reads the old block)
        (void)hipFree(ix->sample_ws);
        ix->sample_ws = nullptr;
        ix->sample_ws_bytes = 0;
        if (hipError_t e = hipMalloc(&ix->sample_ws, off[NT]); e != hipSuccess) {
            (void)hipGetLastError();
            ix->sample_ws = nullptr;
            return fail("hipMalloc of the %zu-byte sampling workspace failed: %s", off[NT], hipGetErrorString(e));
        }
        ix->sample_ws_bytes = off[NT];
    }
    char* tmp[NT];
    for (int i = 0; i < NT; ++i) tmp[i] = (char*)ix->sample_ws + off[i];
    a.p.q_stage = tmp[0];
    a.p.part = tmp[1];
    a.keymax = (float*)tmp[2];
    a.cand_key = tmp[3];
    a.cand_score = (float*)tmp[4];
    a.ctl = (unsigned int*)tmp[5];
    a.status = (unsigned int*)tmp[6];
    hipEvent_t ev[6] = {};
    const bool profile = ix->profile != 0;
    hipError_t le = hipMemsetAsync(a.status, 0, 8 * sizeof(unsigned int), stream);
    if (profile) {
        for (int i = 0; i < 6 && le == hipSuccess; ++i) le = hipEventCreate(&ev[i]);
        a.ev = ev;
    }
    double ns[5] = {0, 0, 0, 0, 0};
    int64_t emit_groups = 0;
    for (int64_t q0 = 0; q0 < nq && le == hipSuccess; q0 += slice) {
        const int64_t n = std::min(slice, nq - q0);
        if (profile) le = hipEventRecord(ev[0], stream);
        if (le == hipSuccess) le = launch_sample_posterior(a, q0, n, stream);
        emit_groups += scan_tiles(a.p.ntotal) * (scan_nq_pad(n) / (n <= 64 ? 64 : 128));
        if (profile && le == hipSuccess) {  // (one slice at a time: the events are reused)
            le = hipEventSynchronize(ev[5]);
            for (int i = 0; i < 5 && le == hipSuccess; ++i) {
                float ms = 0.f;
                le = hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
                ns[i] += (double)ms * 1e6;
            }
        }
    }
    unsigned int st[8] = {};
    if (le == hipSuccess) le = hipMemcpyAsync(st, a.status, sizeof(st), hipMemcpyDeviceToHost, stream);
    if (le != hipSuccess) (void)hipGetLastError();
    const hipError_t se = hipStreamSynchronize(stream);  // the status words have arrived; the workspace is free for the next call
    for (int i = 0; i < 6; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (le != hipSuccess) return fail("sample-posterior launch failed: %s", hipGetErrorString(le));
    HIP_OK(se);
    ix->last_sample[0] = st[0];
    ix->last_sample[1] = st[1];
    ix->last_sample[2] = st[2];
    ix->last_sample[3] = st[3];
    ix->last_sample[4] = (int64_t)(((uint64_t)st[5] << 32) | st[4]);
    ix->last_sample[5] = emit_groups;
    for (int i = 0; i < 5; ++i) ix->last_sample_ns[i] = (int64_t)ns[i];
    if (st[0]) return fail("candidate list overflow: %u queries met more than %d tile maxima tied with their threshold", st[0], VODHIP_SAMPLE_SLACK_TILES);
    return 0;
}

int vodhip_debug_schedule(int64_t ntotal, int k, int64_t nq, int64_t cand_cap, int64_t dense_rows, int64_t sample_div,
                          int64_t growth_x100, int tile, int recovery_pass, int n_cu, int64_t* out, int max_stages) {
    PlanTunables t;
    if (cand_cap > 0) t.cand_cap = cand_cap;
    if (dense_rows > 0) t.dense_rows = round_up(dense_rows, ROW_ALIGN);
    if (sample_div > 0) t.sample_div = sample_div;
    t.growth_x100 = growth_x100;
    t.tile = tile;
    if (n_cu > 0) t.n_cu = n_cu;
    if (!out || max_stages < 1 || k < 1 || nq < 1 || ntotal < 0 || (tile != 0 && !find_kernel(tile) && !experiment_filter(t)))
        return fail("invalid arguments");
    const std::vector<Stage> st = plan_search(ntotal, k, nq, t, false, false, recovery_pass).stages;
    if ((int)st.size() > max_stages) return fail("%d stages do not fit max_stages=%d", (int)st.size(), max_stages);
    for (size_t i = 0; i < st.size(); ++i) {
        const int64_t row[6] = {st[i].kind, st[i].b, st[i].e, st[i].n_tiles, st[i].rstride, st[i].n_groups};
        memcpy(out + i * 6, row, sizeof(row));
    }
    return (int)st.size();
}

int vodhip_debug_tile_order(int64_t ntotal, int64_t* perm_mul, int64_t* perm_mod) {
    if (!perm_mul || !perm_mod || ntotal < 0) return fail("invalid arguments");
    *perm_mod = (ntotal + ROW_ALIGN - 1) / ROW_ALIGN;
    *perm_mul = tile_order_multiplier(*perm_mod);
    return 0;
}

int vodhip_index_set_param(vodhip_index_t* ix, const char* key, int64_t value) {
    if (!ix || !key) return fail("NULL argument");
    if (!strcmp(key, "cand_cap")) {
        if (value < ROW_ALIGN || value > (1 << 16)) return fail("cand_cap must be in [256, 65536]");
        ix->tune.cand_cap = value;
    } else if (!strcmp(key, "dense_rows")) {
        if (value < ROW_ALIGN) return fail("dense_rows must be >= 256");
        ix->tune.dense_rows = round_up(value, ROW_ALIGN);
    } else if (!strcmp(key, "growth")) {
        ix->tune.growth_x100 = value;  // growth factor * 100; 0 = derive from k
    } else if (!strcmp(key, "force_safe")) {
        ix->force_safe = value;
    } else if (!strcmp(key, "small_chunk_tiles")) {
        ix->tune.small_chunk_tiles = value;
    } else if (!strcmp(key, "kflags")) {
        ix->kflags = value;
    } else if (!strcmp(key, "sample_div")) {
        if (value != 0 && value < 2) return fail("sample_div must be 0 (auto) or >= 2");
        ix->tune.sample_div = value;
    } else if (!strcmp(key, "profile")) {
        ix->profile = value;
    } else if (!strcmp(key, "ingest_threads")) {
        if (value < 0 || value > 256) return fail("ingest_threads must be in [0, 256] (0 = auto)");
        ix->ingest_threads = value;
    } else if (!strcmp(key, "lanes")) {
        if (value < 0 || value > 2) return fail("lanes must be 0 (auto: 2 for batches of one query tile), 1 or 2");
        if (!ix->inflight.empty()) return fail("searches are in flight: finish them before changing the lanes");
        ix->lanes = value;
    } else if (!strcmp(key, "survivor_ring")) {
        if (value < 0 || value > MAX_SURVIVOR_RING) return fail("survivor_ring must be in [0, 8192] (0 = auto)");
        ix->tune.survivor_ring = value;
    } else if (!strcmp(key, "tile_order")) {
        if (value != 0 && value != 1) return fail("tile_order must be 0 (low-discrepancy stage order) or 1 (row order)");
        ix->tune.tile_order = value;
    } else if (!strcmp(key, "exact_adapt")) {
        if (value < 0 || value > 1) return fail("exact_adapt must be 0 or 1");
        ix->exact_adapt = value;
        ix->adapt_k = ix->adapt_kx = 0;
    } else if (!strcmp(key, "exact_expand")) {
        if (value < 0 || value > 100000) return fail("exact_expand (x100) must be in [0, 100000]");
        ix->exact_expand_x100 = value;
    } else if (!strcmp(key, "scan_temp_bytes")) {
        if (value < 0) return fail("scan_temp_bytes must be 0 (the default, VODHIP_POSTERIOR_TEMP_BYTES) or >= 1");
        ix->scan_temp_bytes = value == 0 ? VODHIP_POSTERIOR_TEMP_BYTES : value;
    } else if (!strcmp(key, "remove_slab_rows")) {
        if (value != 0 && !remove_slab_rows_ok(value)) return fail("remove_slab_rows must be 0 (the default, 65536) or a power of two in [4, 2^30]");
        ix->remove_slab_rows = value == 0 ? REMOVE_SLAB_ROWS : value;
    } else if (!strcmp(key, "tile")) {
        PlanTunables t;
        t.tile = value;
        if (value != 0 && !find_kernel(value) && !experiment_filter(t))
            return fail("tile must be 0 (auto) or a filter-kernel variant id: 1, 8, 9, 14, 42, 46 (DESIGN.md 4)");
        ix->tune.tile = value;
    } else {
        return fail("unknown parameter '%s'", key);
    }
    return 0;
}

int vodhip_index_get_stat(const vodhip_index_t* ix, const char* key, int64_t* out) {
    if (!ix || !key || !out) return fail("NULL argument");
    if (!strcmp(key, "last_overflow"))
        *out = ix->last_overflow;
    else if (!strcmp(key, "last_chunks"))
        *out = ix->last_chunks;
    else if (!strcmp(key, "last_survivor_ring"))
        *out = ix->last_survivor_ring;
    else if (!strcmp(key, "last_ring_fallbacks"))
        *out = ix->last_ring_fallbacks;
    else if (!strcmp(key, "last_safe_reruns"))
        *out = ix->last_safe_reruns;
    else if (!strcmp(key, "last_recovered_queries"))
        *out = ix->last_recovered_queries;
    else if (!strcmp(key, "last_filter_launches"))
        *out = ix->last_filter_launches;
    else if (!strcmp(key, "last_filter_ns"))
        *out = ix->last_filter_ns;
    else if (!strcmp(key, "last_recovery_launches"))
        *out = ix->last_recovery_launches;
    else if (!strcmp(key, "last_recovery_ns"))
        *out = ix->last_recovery_ns;
    else if (!strcmp(key, "last_sample_overflow"))
        *out = ix->last_sample[0];
    else if (!strcmp(key, "last_sample_selfcheck"))
        *out = ix->last_sample[1];
    else if (!strcmp(key, "last_sample_max_candidates"))
        *out = ix->last_sample[2];
    else if (!strcmp(key, "last_sample_emit_skipped"))
        *out = ix->last_sample[3];
    else if (!strcmp(key, "last_sample_candidates"))
        *out = ix->last_sample[4];
    else if (!strcmp(key, "last_sample_emit_groups"))
        *out = ix->last_sample[5];
    else if (!strcmp(key, "last_range_overflow"))
        *out = ix->last_range[0];
    else if (!strcmp(key, "last_range_selfcheck"))
        *out = ix->last_range[1];
    else if (!strcmp(key, "last_range_emit_skipped"))
        *out = ix->last_range[2];
    else if (!strcmp(key, "last_range_emit_groups"))
        *out = ix->last_range[3];
    else if (!strcmp(key, "last_scan_slice"))
        *out = ix->last_scan[0];
    else if (!strcmp(key, "last_scan_per_query_bytes"))
        *out = ix->last_scan[1];
    else if (!strcmp(key, "scan_temp_bytes"))
        *out = ix->scan_temp_bytes;
    else if (!strcmp(key, "last_sample_ns_partition"))
        *out = ix->last_sample_ns[0];
    else if (!strcmp(key, "last_sample_ns_keymax"))
        *out = ix->last_sample_ns[1];
    else if (!strcmp(key, "last_sample_ns_threshold"))
        *out = ix->last_sample_ns[2];
    else if (!strcmp(key, "last_sample_ns_emit"))
        *out = ix->last_sample_ns[3];
    else if (!strcmp(key, "last_sample_ns_select"))
        *out = ix->last_sample_ns[4];
    else if (!strcmp(key, "exact"))
        *out = ix->exact ? 1 : 0;
    else if (!strcmp(key, "l2"))
        *out = ix->l2 ? 1 : 0;
    else if (!strcmp(key, "last_l2_stage_ns"))
        *out = ix->last_l2_stage_ns;
    else if (!strcmp(key, "last_l2_finish_ns"))
        *out = ix->last_l2_finish_ns;
    else if (!strcmp(key, "l2_saturated_rows")) {  // (waits for the device: ingests on any stream have counted)
        unsigned int w = 0;
        if (ix->l2) {
            HIP_OK(hipSetDevice(ix->device));
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(&w, ix->l2_sat, sizeof(w), hipMemcpyDeviceToHost));
        }
        *out = (int64_t)w;
    } else if (!strcmp(key, "last_update_written") || !strcmp(key, "last_update_skipped") || !strcmp(key, "last_update_duplicates")) {
        // (the last vodhip_index_update_rows; a listed call's two words are read from the device: waits for it, like the count above)
        unsigned int w[2] = {0u, 0u};
        if (ix->last_update_listed) {
            HIP_OK(hipSetDevice(ix->device));
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(w, ix->upd_counts, sizeof(w), hipMemcpyDeviceToHost));
        }
        *out = key[12] == 'w' ? ix->last_update_n - (int64_t)w[0] - (int64_t)w[1] : key[12] == 's' ? (int64_t)w[0] : (int64_t)w[1];
    } else if (!strcmp(key, "last_remove_removed"))
        *out = ix->last_remove[0];
    else if (!strcmp(key, "last_remove_skipped"))
        *out = ix->last_remove[1];
    else if (!strcmp(key, "last_remove_duplicates"))
        *out = ix->last_remove[2];
    else if (!strcmp(key, "remove_slab_rows"))
        *out = ix->remove_slab_rows;
    else if (!strcmp(key, "last_exact_kx"))
        *out = ix->last_exact_kx;
    else if (!strcmp(key, "last_exact_need"))
        *out = ix->last_exact_need;
    else if (!strcmp(key, "exact_outliers")) {  // (derived lazily: before the first search after rows were added this is the previous value)
        *out = ix->n_out;
    } else if (!strcmp(key, "last_exact_band_queries"))
        *out = ix->last_exact_band_queries;
    else if (!strcmp(key, "last_exact_band_passes"))
        *out = ix->last_exact_band_passes;
    else if (!strcmp(key, "cand_cap"))
        *out = ix->tune.cand_cap;
    else if (!strcmp(key, "dense_rows"))
        *out = ix->tune.dense_rows;
    else if (!strcmp(key, "sample_div"))
        *out = ix->tune.sample_div;
    else if (!strcmp(key, "survivor_ring"))
        *out = ix->tune.survivor_ring;
    else if (!strcmp(key, "dim_pad"))
        *out = ix->dim_pad;
    else if (!strcmp(key, "last_ingest_pinned_src"))
        *out = ix->last_ingest_pinned_src;
    else
        return fail("unknown stat '%s'", key);
    return 0;
}

// One merge launch holds n_shards * k entries of a query in LDS (<= 8192).  More than that (e.g. 8 shards x top-2048) is
// merged in levels: groups of floor(8192 / k) shards -> their top-min(k_out, group size * k) in a stream-ordered temporary
// (top-k of a union = top-k of the per-part top-k's), then the groups.
static int merge_topk_levels(const float* scores, int64_t stride_s, const int64_t* ids, int64_t stride_i, int n_shards, int64_t nq,
                             int k, int k_out, float* out_scores, int64_t* out_ids, hipStream_t stream) {
    if ((int64_t)n_shards * k <= 8192) {
        HIP_OK(launch_merge_topk(scores, ids, stride_s, stride_i, n_shards, nq, k, k_out, out_scores, out_ids, stream));
        return 0;
    }
    const int per_group = 8192 / k;
    if (per_group < 2) return fail("k = %d: lists longer than 4096 entries cannot be merged", k);
    const int n_groups = (n_shards + per_group - 1) / per_group;
    const int k_mid = (int)std::min<int64_t>(k_out, (int64_t)per_group * k);
    float* mid_s = nullptr;
    int64_t* mid_i = nullptr;
    const size_t n_mid = (size_t)n_groups * (size_t)nq * (size_t)k_mid;
    HIP_OK(hipMallocAsync((void**)&mid_s, n_mid * sizeof(float), stream));
    if (hipError_t e = hipMallocAsync((void**)&mid_i, n_mid * sizeof(int64_t), stream); e != hipSuccess) {
        (void)hipFreeAsync(mid_s, stream);
        return fail("HIP error: %s", hipGetErrorString(e));
    }
    int rc = 0;
    for (int g = 0; g < n_groups && rc == 0; ++g) {
        const int s0 = g * per_group, ns = std::min(per_group, n_shards - s0);
        if (hipError_t e = launch_merge_topk(scores + (size_t)s0 * stride_s, ids + (size_t)s0 * stride_i, stride_s, stride_i, ns, nq, k, k_mid,
                                             mid_s + (size_t)g * nq * k_mid, mid_i + (size_t)g * nq * k_mid, stream);
            e != hipSuccess)
            rc = fail("HIP error: %s", hipGetErrorString(e));
    }
    if (rc == 0) rc = merge_topk_levels(mid_s, nq * k_mid, mid_i, nq * k_mid, n_groups, nq, k_mid, k_out, out_scores, out_ids, stream);
    (void)hipFreeAsync(mid_s, stream);
    (void)hipFreeAsync(mid_i, stream);
    return rc;
}

int vodhip_merge_topk(const float* scores, const int64_t* ids, int n_shards, int64_t nq, int k, int k_out,
                      float* out_scores, int64_t* out_ids, void* stream) {
    if (n_shards < 1 || k < 1 || k_out < 1 || nq < 0) return fail("invalid sizes");
    if (nq > 0 && (!scores || !ids || !out_scores || !out_ids)) return fail("NULL argument");
    return merge_topk_levels(scores, nq * k, ids, nq * k, n_shards, nq, k, k_out, out_scores, out_ids, (hipStream_t)stream);
}

int vodhip_merge_topk_strided(const float* scores, int64_t shard_stride_scores, const int64_t* ids, int64_t shard_stride_ids,
                              int n_shards, int64_t nq, int k, int k_out, float* out_scores, int64_t* out_ids, void* stream) {
    if (n_shards < 1 || k < 1 || k_out < 1 || nq < 0) return fail("invalid sizes");
    if (nq > 0 && (!scores || !ids || !out_scores || !out_ids)) return fail("NULL argument");
    if (shard_stride_scores < nq * k || shard_stride_ids < nq * k) return fail("shard strides smaller than nq * k");
    return merge_topk_levels(scores, shard_stride_scores, ids, shard_stride_ids, n_shards, nq, k, k_out, out_scores, out_ids,
                             (hipStream_t)stream);
}

int vodhip_merge_hybrid(const int64_t* lookup_idx, const int64_t* lookup_lbl, int k_lookup, int n_engines,
                        const int64_t* const* engine_idx, const float* const* engine_scr, const int* engine_k,
                        const float* engine_weight, int64_t nq, int64_t* out_idx, float* out_scr, int64_t* out_lbl,
                        float* const* out_raw, int out_stride, int32_t* out_width, int32_t* out_row_cursor, void* stream) {
    if (n_engines < 0 || n_engines > VODHIP_MAX_ENGINES) return fail("n_engines=%d out of range", n_engines);
    if (k_lookup < 0 || nq < 0) return fail("invalid sizes");
    HybridArgs a;
    memset(&a, 0, sizeof(a));
    a.lookup_idx = lookup_idx;
    a.lookup_lbl = lookup_lbl;
    a.k_lookup = k_lookup;
    a.n_engines = n_engines;
    int64_t width = k_lookup;
    for (int e = 0; e < n_engines; ++e) {
        if (engine_k[e] < 0 || (engine_k[e] > 0 && (!engine_idx[e] || !engine_scr[e]))) return fail("engine %d: invalid arguments", e);
        a.engine_idx[e] = engine_idx[e];
        a.engine_scr[e] = engine_scr[e];
        a.engine_k[e] = engine_k[e];
        a.engine_w[e] = engine_weight[e];
        a.out_raw[e] = out_raw ? out_raw[e] : nullptr;
        width += engine_k[e];
    }
    if (out_stride < width + 1) return fail("out_stride=%d < %lld", out_stride, (long long)width + 1);
    if (width > 4096) return fail("total width %lld exceeds 4096", (long long)width);
    a.nq = nq;
    a.out_idx = out_idx;
    a.out_scr = out_scr;
    a.out_lbl = out_lbl;
    a.out_stride = out_stride;
    a.out_width = out_width;
    a.out_row_cursor = out_row_cursor;
    if (!out_idx || !out_scr) return fail("NULL output");
    HIP_OK(launch_merge_hybrid(a, (hipStream_t)stream));
    return 0;
}

int vodhip_retrieval_forward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                             const float* score, const int64_t* relevance, const float* sparse, const float* dense,
                             float* retriever_scores, float* d_scores, float* loss, float* kl, float* workspace,
                             void* stream) {
    if (!q || !s || !score || !relevance || !retriever_scores || !d_scores || !loss || !kl || !workspace)
        return fail("NULL argument");
    if (B <= 0 || D <= 0 || H <= 0) return fail("invalid sizes");
    if (D > 16384) return fail("D=%lld exceeds 16384 sections per row", (long long)D);
    if (enc_dtype < 0 || enc_dtype > 2) return fail("invalid enc_dtype");
    HIP_OK(launch_retrieval_forward(q, s, enc_dtype, sections_3d, B, D, H, score, relevance, sparse, dense,
                                    retriever_scores, d_scores, loss, kl, workspace, RetrievalAux(), (hipStream_t)stream));
    return 0;
}

int vodhip_retrieval_forward_aux(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                                 const float* score, const int64_t* relevance, const float* sparse, const float* dense,
                                 int guidance_type, float guidance_weight, float self_supervision_weight, float score_decay,
                                 float* retriever_scores, float* d_scores, float* loss, float* kl, float* aux_losses,
                                 float* aux_grad, float* workspace, int64_t workspace_floats, void* stream) {
    if (workspace_floats < 16 * B) return fail("workspace_floats=%lld < 16 * B", (long long)workspace_floats);
    if (!q || !s || !score || !relevance || !retriever_scores || !d_scores || !loss || !kl || !workspace || !aux_losses)
        return fail("NULL argument");
    if (B <= 0 || D <= 0 || H <= 0) return fail("invalid sizes");
    if (D > 16384) return fail("D=%lld exceeds 16384 sections per row", (long long)D);
    if (enc_dtype < 0 || enc_dtype > 2) return fail("invalid enc_dtype");
    if (guidance_type != 0 && guidance_type != 1) return fail("guidance_type must be 0 (zero) or 1 (sparse)");
    if (guidance_weight < 0 || self_supervision_weight < 0 || score_decay < 0) return fail("negative auxiliary weight");
    const bool any = guidance_weight > 0 || self_supervision_weight > 0 || score_decay > 0;
    if (any && !aux_grad) return fail("aux_grad (3*B*D floats) is required when an auxiliary weight is > 0");
    if (guidance_weight > 0 && guidance_type == 1 && !sparse) return fail("guidance='sparse' needs the sparse scores");
    RetrievalAux aux;
    aux.enabled = 1;
    aux.guidance_type = guidance_type;
    aux.w_guidance = guidance_weight;
    aux.w_self = self_supervision_weight;
    aux.w_decay = score_decay;
    aux.grad = aux_grad;
    aux.out = aux_losses;
    HIP_OK(launch_retrieval_forward(q, s, enc_dtype, sections_3d, B, D, H, score, relevance, sparse, dense,
                                    retriever_scores, d_scores, loss, kl, workspace, aux, (hipStream_t)stream, workspace_floats));
    return 0;
}

int vodhip_retrieval_backward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                              const float* d_scores, const float* grad_out, float* dq, float* ds, void* stream) {
    if (!q || !s || !d_scores || !grad_out || !dq || !ds) return fail("NULL argument");
    if (B <= 0 || D <= 0 || H <= 0) return fail("invalid sizes");
    if (enc_dtype < 0 || enc_dtype > 2) return fail("invalid enc_dtype");
    HIP_OK(launch_retrieval_backward(q, s, enc_dtype, sections_3d, B, D, H, d_scores, grad_out, dq, ds, (hipStream_t)stream));
    return 0;
}

static int marginal_mask_ok(int mask_elem_bytes) {
    return mask_elem_bytes == 1 || mask_elem_bytes == 2 || mask_elem_bytes == 4 || mask_elem_bytes == 8;
}

int vodhip_lm_token_logprob_forward(const void* lm_logits, int logits_dtype, int64_t N, int64_t L, int64_t V,
                                    const int64_t* input_ids, const void* attention_mask, int mask_elem_bytes, float* tok_logp,
                                    float* tok_lse, void* stream) {
    if (!lm_logits || !input_ids || !attention_mask || !tok_logp || !tok_lse) return fail("NULL argument");
    if (N <= 0 || V <= 0) return fail("invalid sizes");
    if (L < 2) return fail("L=%lld: the shifted sequence needs L >= 2", (long long)L);
    if (V > 0x7fffffffLL || N * L > 0x7fffffffLL) return fail("V or N * L exceeds 2^31 - 1");
    if (logits_dtype < 0 || logits_dtype > 2) return fail("invalid logits_dtype");
    if (!marginal_mask_ok(mask_elem_bytes)) return fail("mask_elem_bytes must be 1, 2, 4 or 8");
    HIP_OK(launch_lm_token_forward(lm_logits, logits_dtype, N, L, V, input_ids, attention_mask, mask_elem_bytes, tok_logp, tok_lse,
                                   (hipStream_t)stream));
    return 0;
}

int vodhip_marginal_forward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                            const float* score, const float* tok_logp, const void* attention_mask, int mask_elem_bytes, int64_t L,
                            float* retriever_scores, float* d_scores, float* coef, float* loss, float* workspace,
                            int64_t workspace_floats, void* stream) {
    if (!q || !s || !score || !tok_logp || !attention_mask || !retriever_scores || !d_scores || !coef || !loss || !workspace)
        return fail("NULL argument");
    if (B <= 0 || D <= 0 || H <= 0) return fail("invalid sizes");
    if (L < 2) return fail("L=%lld: the shifted sequence needs L >= 2", (long long)L);
    if (D > 8192) return fail("D=%lld exceeds 8192 sections per row", (long long)D);
    if ((H + 3 * D + 4) * 4 > 160 * 1024) return fail("H + 3 * D = %lld floats exceed the 160 KiB of LDS", (long long)(H + 3 * D));
    if (enc_dtype < 0 || enc_dtype > 2) return fail("invalid enc_dtype");
    if (!marginal_mask_ok(mask_elem_bytes)) return fail("mask_elem_bytes must be 1, 2, 4 or 8");
    if (workspace_floats < B) return fail("workspace_floats=%lld < B", (long long)workspace_floats);
    HIP_OK(launch_marginal_forward(q, s, enc_dtype, sections_3d, B, D, H, score, tok_logp, attention_mask, mask_elem_bytes, L,
                                   retriever_scores, d_scores, coef, loss, workspace, workspace_floats, (hipStream_t)stream));
    return 0;
}

int vodhip_vod_forward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                       const float* score, const float* log_weight, const float* log_proposal, const float* tok_logp,
                       const void* attention_mask, int mask_elem_bytes, int64_t L, double alpha, double temperature,
                       int token_reduction, float* retriever_scores, float* d_scores, float* coef, float* loss, float* diag,
                       float* workspace, int64_t workspace_floats, void* stream) {
    if (!q || !s || !score || !log_weight || !tok_logp || !attention_mask || !retriever_scores || !d_scores || !coef || !loss ||
        !diag || !workspace)
        return fail("NULL argument");
    if (B <= 0 || D <= 0 || H <= 0) return fail("invalid sizes");
    if (L < 2) return fail("L=%lld: the shifted sequence needs L >= 2", (long long)L);
    if (D > 8192) return fail("D=%lld exceeds 8192 sections per row", (long long)D);
    if ((H + 4 * D + 4) * 4 > 160 * 1024) return fail("H + 4 * D = %lld floats exceed the 160 KiB of LDS", (long long)(H + 4 * D));
    if (B > 0x7fffffffLL / 4) return fail("B exceeds 2^29");
    if (enc_dtype < 0 || enc_dtype > 2) return fail("invalid enc_dtype");
    if (!marginal_mask_ok(mask_elem_bytes)) return fail("mask_elem_bytes must be 1, 2, 4 or 8");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail("alpha=%g is outside [0, 1]", alpha);
    if (!std::isfinite(temperature)) return fail("temperature=%g is not finite", temperature);
    if (token_reduction != VODHIP_VOD_TOKEN_MEAN && token_reduction != VODHIP_VOD_TOKEN_SUM)
        return fail("unknown token_reduction (0 = mean, 1 = sum)");
    if (workspace_floats < 4 * B) return fail("workspace_floats=%lld < 4 * B", (long long)workspace_floats);
    HIP_OK(launch_vod_forward(q, s, enc_dtype, sections_3d, B, D, H, score, log_weight, log_proposal, tok_logp, attention_mask,
                              mask_elem_bytes, L, (float)(1.0 - alpha), (float)temperature,
                              token_reduction == VODHIP_VOD_TOKEN_MEAN ? 1 : 0, retriever_scores, d_scores, coef, loss, diag,
                              workspace, workspace_floats, (hipStream_t)stream));
    return 0;
}

int vodhip_lm_token_logprob_backward(const void* lm_logits, int logits_dtype, int64_t N, int64_t L, int64_t V,
                                     const int64_t* input_ids, const void* attention_mask, int mask_elem_bytes,
                                     const float* tok_lse, const float* coef, const float* grad_out, void* d_logits, void* stream) {
    if (!lm_logits || !input_ids || !attention_mask || !tok_lse || !coef || !grad_out || !d_logits) return fail("NULL argument");
    if (N <= 0 || V <= 0) return fail("invalid sizes");
    if (L < 2) return fail("L=%lld: the shifted sequence needs L >= 2", (long long)L);
    if (V > 0x7fffffffLL || N * L > 0x7fffffffLL) return fail("V or N * L exceeds 2^31 - 1");
    if (logits_dtype < 0 || logits_dtype > 2) return fail("invalid logits_dtype");
    if (!marginal_mask_ok(mask_elem_bytes)) return fail("mask_elem_bytes must be 1, 2, 4 or 8");
    HIP_OK(launch_lm_token_backward(lm_logits, logits_dtype, N, L, V, input_ids, attention_mask, mask_elem_bytes, tok_lse, coef,
                                    grad_out, d_logits, (hipStream_t)stream));
    return 0;
}

static const char* pool_codes_error(int agg, int mask_mode, int act, int norm) {
    if (agg != VODHIP_POOL_AGG_MEAN && agg != VODHIP_POOL_AGG_CLS) return "unknown aggregator code (0 = mean, 1 = cls)";
    if (mask_mode != VODHIP_POOL_MASK_REFERENCE && mask_mode != VODHIP_POOL_MASK_MASKED) return "unknown mask_mode (0 = reference, 1 = masked)";
    if (act < VODHIP_POOL_ACT_NONE || act > VODHIP_POOL_ACT_GELU) return "unknown activation code (0 none, 1 relu, 2 tanh, 3 sigmoid, 4 gelu)";
    if (norm < VODHIP_POOL_NORM_NONE || norm > VODHIP_POOL_NORM_L1) return "unknown norm code (0 none, 1 l2, 2 l1)";
    return nullptr;
}
static const char* pool_sizes_error(int64_t N, int64_t L, int64_t H, int64_t l_chunk) {
    if (N <= 0 || L <= 0 || H <= 0 || l_chunk < 0) return "invalid sizes";
    if (H > (1LL << 30)) return "H exceeds 2^30";
    if (L > 0x7fffffffLL || N > 0x7fffffffLL / L) return "N * L exceeds 2^31 - 1";
    return nullptr;
}
static bool pool_dtype_ok(int dt) { return dt >= 0 && dt <= 2; }

int64_t vodhip_pool_workspace_floats(int64_t N, int64_t L, int64_t H, int64_t l_chunk) {
    if (const char* m = pool_sizes_error(N, L, H, l_chunk)) return fail("%s", m);
    const PoolPlan plan = pool_plan(N, L, H, l_chunk);
    return plan.n_chunks == 1 ? 0 : N * plan.n_chunks * H;
}

int vodhip_pool_forward(const void* hidden, int hidden_dtype, int64_t N, int64_t L, int64_t H, const void* attention_mask,
                        int mask_elem_bytes, int agg, int mask_mode, int finish, int act, int norm, const float* log_scaler,
                        int64_t l_chunk, float* a, void* y, int y_dtype, float* workspace, int64_t workspace_floats, void* stream) {
    if (!hidden || !attention_mask || !a || (finish && (!y || !log_scaler))) return fail("NULL argument");
    if (const char* m = pool_sizes_error(N, L, H, l_chunk)) return fail("%s", m);
    if (!pool_dtype_ok(hidden_dtype)) return fail("invalid hidden_dtype");
    if (finish && !pool_dtype_ok(y_dtype)) return fail("invalid y_dtype");
    if (!marginal_mask_ok(mask_elem_bytes)) return fail("mask_elem_bytes must be 1, 2, 4 or 8");
    if (const char* m = pool_codes_error(agg, mask_mode, act, norm)) return fail("%s", m);
    const PoolPlan plan = pool_plan(N, L, H, l_chunk);
    if (agg == VODHIP_POOL_AGG_MEAN && plan.n_chunks > 1) {
        const int64_t need = N * plan.n_chunks * H;
        if (!workspace || workspace_floats < need)
            return fail("workspace_floats=%lld < %lld (N * %lld chunks * H)", (long long)workspace_floats, (long long)need,
                        (long long)plan.n_chunks);
    }
    HIP_OK(launch_pool_forward(hidden, hidden_dtype, N, L, H, attention_mask, mask_elem_bytes, agg, mask_mode, finish ? 1 : 0, act, norm,
                               log_scaler, l_chunk, a, y, y_dtype, workspace, (hipStream_t)stream));
    return 0;
}

int vodhip_pool_backward(const void* g, int g_dtype, const float* a, int64_t N, int64_t L, int64_t H, const void* attention_mask,
                         int mask_elem_bytes, int agg, int mask_mode, int finish, int act, int norm, const float* log_scaler,
                         int64_t l_chunk, void* d_hidden, int hidden_dtype, float* gy, void* stream) {
    if (!g || !attention_mask || !d_hidden || (finish && (!a || !log_scaler || !gy))) return fail("NULL argument");
    if (const char* m = pool_sizes_error(N, L, H, l_chunk)) return fail("%s", m);
    if (!pool_dtype_ok(hidden_dtype)) return fail("invalid hidden_dtype");
    if (!pool_dtype_ok(g_dtype)) return fail("invalid g_dtype");
    if (!marginal_mask_ok(mask_elem_bytes)) return fail("mask_elem_bytes must be 1, 2, 4 or 8");
    if (const char* m = pool_codes_error(agg, mask_mode, act, norm)) return fail("%s", m);
    HIP_OK(launch_pool_backward(g, g_dtype, a, N, L, H, attention_mask, mask_elem_bytes, agg, mask_mode, finish ? 1 : 0, act, norm,
                                log_scaler, l_chunk, d_hidden, hidden_dtype, gy, (hipStream_t)stream));
    return 0;
}

int vodhip_pool_finish_forward(const void* z, int z_dtype, int64_t N, int64_t P, int act, int norm, const float* log_scaler, void* y,
                               int y_dtype, void* stream) {
    if (!z || !log_scaler || !y) return fail("NULL argument");
    if (N <= 0 || P <= 0 || N > 0x7fffffffLL || P > (1LL << 30)) return fail("invalid sizes");
    if (!pool_dtype_ok(z_dtype) || !pool_dtype_ok(y_dtype)) return fail("invalid z_dtype or y_dtype");
    if (const char* m = pool_codes_error(VODHIP_POOL_AGG_MEAN, VODHIP_POOL_MASK_REFERENCE, act, norm)) return fail("%s", m);
    HIP_OK(launch_pool_finish_forward(z, z_dtype, N, P, act, norm, log_scaler, y, y_dtype, (hipStream_t)stream));
    return 0;
}

int vodhip_pool_finish_backward(const void* z, int z_dtype, const void* g, int g_dtype, int64_t N, int64_t P, int act, int norm,
                                const float* log_scaler, void* dz, int dz_dtype, float* gy, void* stream) {
    if (!z || !g || !log_scaler || !dz || !gy) return fail("NULL argument");
    if (N <= 0 || P <= 0 || N > 0x7fffffffLL || P > (1LL << 30)) return fail("invalid sizes");
    if (!pool_dtype_ok(z_dtype) || !pool_dtype_ok(g_dtype) || !pool_dtype_ok(dz_dtype)) return fail("invalid z_dtype, g_dtype or dz_dtype");
    if (const char* m = pool_codes_error(VODHIP_POOL_AGG_MEAN, VODHIP_POOL_MASK_REFERENCE, act, norm)) return fail("%s", m);
    HIP_OK(launch_pool_finish_backward(z, z_dtype, g, g_dtype, N, P, act, norm, log_scaler, dz, dz_dtype, gy, (hipStream_t)stream));
    return 0;
}

int vodhip_retrieval_metrics(const float* scores, const int64_t* relevances, int64_t B, int width, const int32_t* specs, int n_specs,
                             float* values, double* state, void* workspace, int64_t workspace_bytes, void* stream) {
    if (B <= 0 || width <= 0) return fail("invalid sizes B=%lld width=%d", (long long)B, width);
    if (width > 4096) return fail("width=%d exceeds 4096 candidates per row", width);
    if (n_specs < 1 || n_specs > VODHIP_MAX_METRIC_SPECS) return fail("n_specs=%d is outside 1..%d", n_specs, VODHIP_MAX_METRIC_SPECS);
    if (!scores || !relevances || !specs) return fail("NULL argument");
    if (!values && !state) return fail("values and state are both NULL: nothing to compute");
    MetricSpecs ms{};
    ms.n = n_specs;
    for (int i = 0; i < n_specs; ++i) {
        const int metric = specs[2 * i], topk = specs[2 * i + 1];
        if (metric < VODHIP_METRIC_MRR || metric > VODHIP_METRIC_ENTROPY) return fail("spec %d: unknown metric id %d", i, metric);
        if (topk < 0) return fail("spec %d: topk=%d is negative (0 = no cut)", i, topk);
        ms.metric[i] = metric;
        ms.topk[i] = topk;
    }
    if (!values) {  // the per-row values live in the caller's workspace
        const int64_t need = (int64_t)n_specs * B * (int64_t)sizeof(float);
        if (!workspace || workspace_bytes < need)
            return fail("workspace_bytes=%lld < %lld (n_specs * B floats, needed when values is NULL)", (long long)workspace_bytes, (long long)need);
        values = (float*)workspace;
    }
    HIP_OK(launch_retrieval_metrics(scores, relevances, B, width, ms, values, state, (hipStream_t)stream));
    return 0;
}

static int priority_sample_impl(const float* scores, const uint8_t* labels, const float* noise, int64_t nq, int width,
                                int k_positive, int k_total, float temperature, int max_support_size, int normalized,
                                int64_t* out_samples, float* out_log_weights, uint8_t* out_labels, float* out_lse,
                                float* out_log_proposal, float* out_log_mass, float* out_joint_log_weights, void* stream) {
    if (nq < 0 || width < 0 || k_total < 1 || k_positive < 0) return fail("invalid sizes");
    if (width > 4096) return fail("width=%d exceeds 4096 candidates per row", width);
    if (k_total > 4096) return fail("k_total=%d exceeds 4096", k_total);
    if (out_joint_log_weights && !(normalized & 1)) return fail("out_joint_log_weights needs the `normalized` bit: the joint weights re-scale the self-normalised ones");
    if (nq == 0) return 0;
    if (!scores || !labels || !noise || !out_samples || !out_log_weights || !out_labels || !out_lse) return fail("NULL argument");
    HIP_OK(launch_priority_sample(scores, labels, noise, nq, width, k_positive, k_total, temperature, max_support_size,
                                  normalized, out_samples, out_log_weights, out_labels, out_lse, out_log_proposal, out_log_mass,
                                  out_joint_log_weights, (hipStream_t)stream));
    return 0;
}

int vodhip_priority_sample(const float* scores, const uint8_t* labels, const float* noise, int64_t nq, int width,
                           int k_positive, int k_total, float temperature, int max_support_size, int normalized,
                           int64_t* out_samples, float* out_log_weights, uint8_t* out_labels, float* out_lse,
                           void* stream) {
    return priority_sample_impl(scores, labels, noise, nq, width, k_positive, k_total, temperature, max_support_size, normalized,
                                out_samples, out_log_weights, out_labels, out_lse, nullptr, nullptr, nullptr, stream);
}

int vodhip_priority_sample_proposal(const float* scores, const uint8_t* labels, const float* noise, int64_t nq, int width,
                                    int k_positive, int k_total, float temperature, int max_support_size, int normalized,
                                    int64_t* out_samples, float* out_log_weights, uint8_t* out_labels, float* out_lse,
                                    float* out_log_proposal, float* out_log_mass, float* out_joint_log_weights, void* stream) {
    return priority_sample_impl(scores, labels, noise, nq, width, k_positive, k_total, temperature, max_support_size, normalized,
                                out_samples, out_log_weights, out_labels, out_lse, out_log_proposal, out_log_mass,
                                out_joint_log_weights, stream);
}

static int priority_sample_merged_impl(const int64_t* ids, const float* scores, const int64_t* labels, int n_raw, const float* const* raw,
                                       const float* noise, int64_t noise_stride, int64_t nq, int stride, int width,
                                       const int32_t* merge_width, const int32_t* merge_row_cursor, int k_lookup, int n_engines,
                                       const int* engine_k, int k_positive,
                                       int k_total, float temperature, int max_support_size, int normalized, int64_t* out_samples,
                                       int64_t* out_ids, float* out_scores, float* out_log_weights, uint8_t* out_labels,
                                       float* const* out_raw, float* out_lse, float* out_max_sampling_id, float* out_log_proposal,
                                       float* out_log_mass, float* out_joint_log_weights, void* stream) {
    if (out_joint_log_weights && !(normalized & 1)) return fail("out_joint_log_weights needs the `normalized` bit: the joint weights re-scale the self-normalised ones");
    if (nq < 0 || stride < 0 || k_total < 1 || k_positive < 0) return fail("invalid sizes");
    if (stride > 4096 || width > stride) return fail("stride=%d / width=%d: at most 4096 candidates per row, width <= stride", stride, width);
    if (k_total > 4096) return fail("k_total=%d exceeds 4096", k_total);
    if (n_raw < 0 || n_raw > VODHIP_MAX_ENGINES || (n_raw && (!raw || !out_raw))) return fail("n_raw=%d out of range / NULL raw arrays", n_raw);
    if (noise_stride < (width >= 0 ? width : stride)) return fail("noise rows are shorter than the candidate rows");
    if (nq == 0) return 0;
    if (!ids || !scores || !labels || !noise || !out_samples || !out_ids || !out_scores || !out_log_weights || !out_labels || !out_lse)
        return fail("NULL argument");
    SampleMergedArgs m{};
    if (width < 0) {
        if ((n_engines > 0 && !merge_width && !merge_row_cursor) || !engine_k || n_engines < 0 || n_engines > VODHIP_MAX_ENGINES || k_lookup < 0)
            return fail("width < 0 needs merge_width or merge_row_cursor, k_lookup and engine_k of the merge that produced the rows");
        int64_t w_max = k_lookup;
        for (int e = 0; e < n_engines; ++e) {
            if (engine_k[e] < 0) return fail("engine %d: negative k", e);
            m.engine_k[e] = engine_k[e];
            w_max += engine_k[e];
        }
        if (n_engines > 0 && stride < w_max + 1) return fail("stride=%d < k_lookup + sum(k_e) + 1 = %lld", stride, (long long)w_max + 1);
        if (n_engines == 0 && stride < w_max) return fail("stride=%d < k_lookup", stride);
    }
    m.ids = ids;
    m.scores = scores;
    m.labels = labels;
    m.noise = noise;
    m.nq = nq;
    m.stride = stride;
    m.noise_stride = noise_stride;
    m.width = width;
    m.merge_width = merge_width;
    m.row_cursor = merge_row_cursor;
    m.k_lookup = k_lookup;
    m.n_engines = width < 0 ? n_engines : 0;
    m.k_positive = k_positive;
    m.k_total = k_total;
    m.temperature = temperature;
    m.max_support = max_support_size;
    m.normalized = normalized;
    m.n_raw = n_raw;
    for (int e = 0; e < n_raw; ++e) {
        if (!raw[e] || !out_raw[e]) return fail("NULL raw array %d", e);
        m.raw[e] = raw[e];
        m.out_raw[e] = out_raw[e];
    }
    m.out_samples = out_samples;
    m.out_ids = out_ids;
    m.out_scores = out_scores;
    m.out_logw = out_log_weights;
    m.out_labels = out_labels;
    m.out_lse = out_lse;
    m.lse_row_stride = 2;
    m.lse_cls_stride = 1;
    m.out_max_sampling_id = out_max_sampling_id;
    m.out_log_proposal = out_log_proposal;
    m.out_log_mass = out_log_mass;
    m.mass_cls_stride = 1;
    m.out_joint_logw = out_joint_log_weights;
    HIP_OK(launch_priority_sample_merged(m, (hipStream_t)stream));
    return 0;
}

int vodhip_priority_sample_merged(const int64_t* ids, const float* scores, const int64_t* labels, int n_raw, const float* const* raw,
                                  const float* noise, int64_t noise_stride, int64_t nq, int stride, int width,
                                  const int32_t* merge_width, const int32_t* merge_row_cursor, int k_lookup, int n_engines,
                                  const int* engine_k, int k_positive,
                                  int k_total, float temperature, int max_support_size, int normalized, int64_t* out_samples,
                                  int64_t* out_ids, float* out_scores, float* out_log_weights, uint8_t* out_labels,
                                  float* const* out_raw, float* out_lse, float* out_max_sampling_id, void* stream) {
    return priority_sample_merged_impl(ids, scores, labels, n_raw, raw, noise, noise_stride, nq, stride, width, merge_width,
                                       merge_row_cursor, k_lookup, n_engines, engine_k, k_positive, k_total, temperature,
                                       max_support_size, normalized, out_samples, out_ids, out_scores, out_log_weights, out_labels,
                                       out_raw, out_lse, out_max_sampling_id, nullptr, nullptr, nullptr, stream);
}

int vodhip_priority_sample_merged_proposal(const int64_t* ids, const float* scores, const int64_t* labels, int n_raw,
                                           const float* const* raw, const float* noise, int64_t noise_stride, int64_t nq, int stride,
                                           int width, const int32_t* merge_width, const int32_t* merge_row_cursor, int k_lookup,
                                           int n_engines, const int* engine_k, int k_positive, int k_total, float temperature,
                                           int max_support_size, int normalized, int64_t* out_samples, int64_t* out_ids,
                                           float* out_scores, float* out_log_weights, uint8_t* out_labels, float* const* out_raw,
                                           float* out_lse, float* out_max_sampling_id, float* out_log_proposal, float* out_log_mass,
                                           float* out_joint_log_weights, void* stream) {
    return priority_sample_merged_impl(ids, scores, labels, n_raw, raw, noise, noise_stride, nq, stride, width, merge_width,
                                       merge_row_cursor, k_lookup, n_engines, engine_k, k_positive, k_total, temperature,
                                       max_support_size, normalized, out_samples, out_ids, out_scores, out_log_weights, out_labels,
                                       out_raw, out_lse, out_max_sampling_id, out_log_proposal, out_log_mass, out_joint_log_weights,
                                       stream);
}

// The one-launch flattening's admitted shapes (collate_plan.h, flatten_admits): 0 = admitted; otherwise the refusal is recorded
static int flatten_refused(int64_t n_rows, int64_t n_keys) {
    if (n_keys > 0 && n_rows > FL_MAX_IDS / n_keys)
        return fail("%lld rows of %lld ids: the one-launch flattening holds at most %d ids in the batch", (long long)n_rows, (long long)n_keys, FL_MAX_IDS);
    if (n_keys > FL_MAX_KEYS)
        return fail("%lld ids per row: the one-launch flattening stages at most %d per row in LDS (use vodhip_gather_by_id)", (long long)n_keys, FL_MAX_KEYS);
    if (!flatten_admits(n_rows, n_keys))
        return fail("%lld rows of %lld ids: the one-launch flattening needs %zu bytes of LDS, one workgroup has %zu - 8 rows hold at most 1012 ids each (use vodhip_gather_by_id)",
                    (long long)n_rows, (long long)n_keys, flatten_plan(n_rows, (int)n_keys).lds, CL_LDS_LIMIT);
    return 0;
}

int vodhip_flatten_inbatch_admits(int64_t n_rows, int n_keys) { return flatten_admits(n_rows, n_keys) ? 1 : 0; }

int vodhip_flatten_inbatch(const int64_t* ids, int64_t n_rows, int n_keys, int n_values, const float* const* values, const float* fill,
                           float* const* outs, const uint8_t* labels, uint8_t* out_labels, int64_t* out_unique, int32_t* out_n_unique,
                           void* stream) {
    if (n_rows < 0 || n_keys < 0 || n_values < 0 || n_values > 8) return fail("invalid sizes (n_values <= 8)");
    if ((labels == nullptr) != (out_labels == nullptr)) return fail("labels and out_labels go together");
    if (flatten_refused(n_rows, n_keys)) return -1;
    if (n_rows == 0 || n_keys == 0) return 0;
    if (!ids || !out_unique || (n_values && (!values || !fill || !outs))) return fail("NULL argument");
    for (int v = 0; v < n_values; ++v)
        if (!outs[v] || !values[v]) return fail("NULL value / output array %d", v);
    HIP_OK(launch_flatten_inbatch(ids, n_rows, n_keys, n_values, values, fill, outs, labels, out_labels, out_unique, out_n_unique,
                                  (hipStream_t)stream));
    return 0;
}

// `p`: the proposal outputs of vodhip_collate_proposal (NULL: plain vodhip_collate)
static int collate_impl(const vodhip_collate_args_t* c, const vodhip_collate_proposal_args_t* p, void* stream_) {
    if (!c) return fail("args is NULL");
    float* const out_logp = p ? p->out_log_proposal : nullptr;
    float* const out_joint = p ? p->out_joint_log_weights : nullptr;
    float* const flat_logp = p ? p->flat_log_proposal : nullptr;
    float* const flat_joint = p ? p->flat_joint_log_weights : nullptr;
    if (p) {
        if ((p->out_log_mass_pos == nullptr) != (p->out_log_mass_neg == nullptr)) return fail("out_log_mass_pos and out_log_mass_neg go together");
        if ((flat_logp && !out_logp) || (flat_joint && !out_joint)) return fail("a flattened proposal output needs its [nq, k_total] source output");
        if ((flat_logp || flat_joint) && !c->in_batch_negatives) return fail("flattened proposal outputs need in_batch_negatives");
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (c->n_engines < 1 || c->n_engines > VODHIP_MAX_ENGINES) return fail("n_engines=%d out of range [1, %d]", c->n_engines, VODHIP_MAX_ENGINES);
    if (c->k_lookup < 0 || c->nq < 0 || c->k_total < 1 || c->k_positive < 0) return fail("invalid sizes");
    int64_t stride = c->k_lookup + 1;
    for (int e = 0; e < c->n_engines; ++e) {
        if (c->engine_k[e] < 0 || (c->engine_k[e] > 0 && (!c->engine_idx[e] || !c->engine_scr[e]))) return fail("engine %d: invalid arguments", e);
        if (!c->merged_raw[e] || !c->out_raw[e]) return fail("engine %d: NULL raw-score workspace / output", e);
        stride += c->engine_k[e];
    }
    if (stride - 1 > 4096) return fail("total width %lld exceeds 4096", (long long)stride - 1);
    if (c->k_total > 4096) return fail("k_total=%d exceeds 4096", c->k_total);
    if (c->noise_stride < stride) return fail("noise rows (%lld) are shorter than the merged rows (%lld)", (long long)c->noise_stride, (long long)stride);
    if (c->in_batch_negatives && flatten_refused(c->nq, c->k_total)) return -1;  // before anything is launched
    if (c->nq == 0) return 0;
    if ((c->k_lookup && !c->lookup_idx) || !c->noise || !c->merged_idx || !c->merged_lbl || !c->merged_scr || !c->row_cursor || !c->out_local ||
        !c->out_ids || !c->out_scores || !c->out_log_weights || !c->out_labels || !c->out_lse_pos || !c->out_lse_neg)
        return fail("NULL argument");
    HybridArgs h;
    memset(&h, 0, sizeof(h));
    h.lookup_idx = c->lookup_idx;
    h.lookup_lbl = c->lookup_lbl;
    h.k_lookup = c->k_lookup;
    h.n_engines = c->n_engines;
    for (int e = 0; e < c->n_engines; ++e) {
        h.engine_idx[e] = c->engine_idx[e];
        h.engine_scr[e] = c->engine_scr[e];
        h.engine_k[e] = c->engine_k[e];
        h.engine_w[e] = c->engine_weight[e];
        h.out_raw[e] = c->merged_raw[e];
    }
    h.nq = c->nq;
    h.out_idx = c->merged_idx;
    h.out_scr = c->merged_scr;
    h.out_lbl = c->merged_lbl;
    h.out_stride = (int)stride;
    h.out_row_cursor = c->row_cursor;
    HIP_OK(launch_merge_hybrid(h, stream));
    SampleMergedArgs m{};
    m.ids = c->merged_idx;
    m.scores = c->merged_scr;
    m.labels = c->merged_lbl;
    m.noise = c->noise;
    m.nq = c->nq;
    m.stride = stride;
    m.noise_stride = c->noise_stride;
    m.width = -1;
    m.row_cursor = c->row_cursor;
    m.k_lookup = c->k_lookup;
    m.n_engines = c->n_engines;
    m.n_raw = c->n_engines;
    for (int e = 0; e < c->n_engines; ++e) {
        m.engine_k[e] = c->engine_k[e];
        m.raw[e] = c->merged_raw[e];
        m.out_raw[e] = c->out_raw[e];
    }
    m.k_positive = c->k_positive;
    m.k_total = c->k_total;
    m.temperature = c->temperature;
    m.max_support = c->max_support_size;
    m.normalized = 1 | (c->flags & VODHIP_SAMPLE_KEEP_TOP_SUPPORT);
    m.out_samples = c->out_local;
    m.out_ids = c->out_ids;
    m.out_scores = c->out_scores;
    m.out_logw = c->out_log_weights;
    m.out_labels = c->out_labels;
    // lse_pos / lse_neg are two [nq] arrays: class stride = their distance (any two arrays of the same type can be addressed so)
    m.out_lse = c->out_lse_pos;
    m.lse_row_stride = 1;
    m.lse_cls_stride = c->out_lse_neg - c->out_lse_pos;
    m.out_max_sampling_id = c->out_max_sampling_id;
    if (p) {
        m.out_log_proposal = out_logp;
        m.out_log_mass = p->out_log_mass_pos;  // two [nq] arrays, addressed like lse_pos / lse_neg
        m.mass_cls_stride = p->out_log_mass_pos ? p->out_log_mass_neg - p->out_log_mass_pos : 0;
        m.out_joint_logw = out_joint;  // (the collate always samples with the `normalized` bit)
    }
    HIP_OK(launch_priority_sample_merged(m, stream));
    if (!c->in_batch_negatives) return 0;
    if (!c->flat_ids || !c->flat_scores || !c->flat_log_weights || !c->flat_labels) return fail("NULL flattened output");
    const float* values[8];
    float* outs[8];
    float fill[8];
    int nv = 0;
    values[nv] = c->out_scores, outs[nv] = c->flat_scores, fill[nv++] = __builtin_nanf("");
    values[nv] = c->out_log_weights, outs[nv] = c->flat_log_weights, fill[nv++] = __builtin_nanf("");
    for (int e = 0; e < c->n_engines; ++e) {
        if (!c->flat_raw[e]) return fail("engine %d: NULL flattened raw-score output", e);
        values[nv] = c->out_raw[e], outs[nv] = c->flat_raw[e], fill[nv++] = __builtin_nanf("");
    }
    // the proposal arrays fill with -inf: "this row did not sample the id" is weight 0 for the objective, not NaN
    if (nv + (flat_logp != nullptr) + (flat_joint != nullptr) > 8) return fail("%d value arrays to flatten: the one-launch flattening carries at most 8", nv + (flat_logp != nullptr) + (flat_joint != nullptr));
    if (flat_logp) values[nv] = out_logp, outs[nv] = flat_logp, fill[nv++] = -__builtin_inff();
    if (flat_joint) values[nv] = out_joint, outs[nv] = flat_joint, fill[nv++] = -__builtin_inff();
    HIP_OK(launch_flatten_inbatch(c->out_ids, c->nq, c->k_total, nv, values, fill, outs, c->out_labels, c->flat_labels, c->flat_ids,
                                  c->flat_n_unique, stream));
    return 0;
}

int vodhip_collate(const vodhip_collate_args_t* args, void* stream) { return collate_impl(args, nullptr, stream); }

int vodhip_collate_proposal(const vodhip_collate_proposal_args_t* args, void* stream) {
    if (!args) return fail("args is NULL");
    return collate_impl(&args->base, args, stream);
}

int vodhip_gather_by_id(const int64_t* queries, int64_t n_queries, const int64_t* keys, int64_t n_rows, int n_keys,
                        int n_values, const float* const* values, const float* fill, float* const* outs, void* stream) {
    if (n_queries < 0 || n_rows < 0 || n_keys < 0 || n_values < 1 || n_values > 8) return fail("invalid sizes (1 <= n_values <= 8)");
    if (n_keys > 4096) return fail("n_keys=%d exceeds 4096 candidates per row", n_keys);
    if (n_queries >= (1ll << 31)) return fail("too many query ids");
    if (n_queries == 0 || n_rows == 0) return 0;
    if (!queries || !values || !fill || !outs || (n_keys && !keys)) return fail("NULL argument");
    for (int v = 0; v < n_values; ++v)
        if (!outs[v] || (n_keys && !values[v])) return fail("NULL value / output array %d", v);
    HIP_OK(launch_gather_by_id(queries, n_queries, keys, n_rows, n_keys, n_values, values, fill, outs, (hipStream_t)stream));
    return 0;
}

int vodhip_debug_read_probe(int which, int64_t* out, int n) {
    if (!out || n < 256) return fail("out must hold 256 values");
    static_assert(sizeof(long long) == sizeof(int64_t), "probe words are 64-bit");
    const hipError_t e = which == 0 ? read_probe_hybrid((long long*)out) : which == 3 ? read_probe_select((long long*)out) : read_probe_sample(which, (long long*)out);
    if (e == hipErrorNotSupported) return fail("phase stamps exist in diagnostic builds only (make ABLATION=1)");
    if (e != hipSuccess) return fail("HIP error: %s", hipGetErrorString(e));
    return 0;
}

// (the wire codec - vodhip_b64url_encode / vodhip_b64url_decode - lives in wire_codec.cpp: host C++ with AVX2 paths)

}  // extern "C"

// ---- what the node form of the key gradient needs of a shard beyond the C-ABI (vodhip_internal.h) ----
namespace vodhip {

int index_value_vmax(vodhip_index* ix, float* vmax_host, int64_t c_pad, hipStream_t stream) {
    if (!ix || !ix->row_value || ix->value_c_pad != c_pad) return fail("posterior_key_gradient: the shard holds no value table of that width");
    HIP_OK(hipSetDevice(ix->device));
    if (ensure_value_vmax(ix, "posterior-key-gradient", stream)) return -1;
    HIP_OK(hipMemcpyAsync(vmax_host, ix->value_vmax, (size_t)c_pad * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
}

int index_posterior_key_gradient(vodhip_index* ix, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels_dev, int n_per_query,
                                 const float* max_score, const float* log_rel, const float* grad_log_z, const float* values, const float* grad_values,
                                 const float* vmax_dev, float* out, hipStream_t stream) {
    return index_key_gradient(ix, queries, q_dtype, nq, beta, q_labels_dev, n_per_query, max_score, log_rel, grad_log_z, values, grad_values, vmax_dev, 0, out, stream);
}

}  // namespace vodhip
