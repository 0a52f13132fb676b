// vodhip_node_index_*: the row-sharded index of ONE node driven from ONE process, for consumers that have no
// torch.distributed (C, C++, cgo, JNI): every device holds a contiguous row range, a search runs on all devices at once and the
// per-shard top-k lists meet on devices[0] (peer copies over xGMI) where vodhip_merge_topk folds them.
// Counterpart of faiss.index_cpu_to_all_gpus(index, co) with co.shard = True (/root/reference/src/vod_search/faiss_search/
// server.py:51-54, vod_configs/search.py:80).  A composition of the PUBLIC entry points of include/vodhip.h - nothing here reaches
// into a shard's internals.  (The Python host shards with one process per GPU and one RCCL all-gather instead: vod_amd/distributed.py.)
#include "../../include/vodhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

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
#include "vodhip_internal.h"

namespace {

int nfail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    vodhip::set_last_error(buf);
    return -1;
}

#define NODE_HIP_OK(expr)                                                                                               \
    do {                                                                                                                \
        hipError_t _e = (expr);                                                                                         \
        if (_e != hipSuccess) {                                                                                         \
            (void)hipGetLastError();                                                                                    \
            return nfail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);                   \
        }                                                                                                               \
    } while (0)

inline size_t elem_bytes(int dtype) { return dtype == VODHIP_F32 ? 4 : 2; }

struct ShardBuffers {
    void* q = nullptr;          // the query batch on this shard's device
    float* scores = nullptr;    // this shard's top-k [nq, k]
    int64_t* ids = nullptr;
    int32_t* q_labels = nullptr;  // the batch's allowed subset labels on this shard's device
    size_t q_bytes = 0, res_elems = 0, q_label_elems = 0;
};

}  // namespace

// Everything ONE search in flight owns (round 6: two slots, so that the host enqueues batch i + 1 on every shard - 7 launches per shard -
// while batch i runs: with 8 shards the enqueue alone is ~0.3 ms of host time per batch, which a synchronous search adds to every step)
struct NodeSlot {
    std::vector<ShardBuffers> buf;     // per shard: queries, top-k list, subset labels on its device
    std::vector<hipEvent_t> arrived;   // shard g's result is on devices[0]
    hipEvent_t ready = nullptr;        // on devices[0]: the caller's queries are readable / the slot's previous merge has read `gathered`
    float* gathered_scores = nullptr;  // devices[0]: [n, nq, k]
    int64_t* gathered_ids = nullptr;
    float* merged_scores = nullptr;    // devices[0]: [nq, k] (host-located outputs)
    int64_t* merged_ids = nullptr;
    size_t gathered_elems = 0, merged_elems = 0;
    std::vector<void*> pin_res;        // per shard: pinned [scores f32 | ids i64] of its top-k list (host-staged route)
    std::vector<size_t> pin_res_elems;
    std::vector<hipEvent_t> on_host;   // shard g's list is in pin_res[g]
    void* pin_q = nullptr;             // the query batch (+ subset labels) staged from devices[0]
    size_t pin_q_bytes = 0;
    hipEvent_t q_on_host = nullptr;
    hipEvent_t merge_ev[2] = {nullptr, nullptr};   // param "profile": on devices[0]
    std::vector<hipEvent_t> copy_ev;               // [2 * n]: begin / end of shard g's copy, on its device
    bool timed = false;                            // the events above belong to this slot's last search
    std::vector<char> enqueued;        // shard g holds this slot's search in its FIFO (drained if a call fails half-way)
    // the search in flight
    bool pending = false;
    int64_t nq = 0;
    int k = 0, location = 0;
    float* out_scores = nullptr;
    int64_t* out_ids = nullptr;
    hipStream_t user = nullptr;
};

struct vodhip_node_index {
    int n = 0;
    int64_t dim = 0, capacity = 0, rows_per_shard = 0, ntotal = 0;
    int dtype = 0;
    std::vector<int> device;
    std::vector<vodhip_index_t*> shard;
    std::vector<hipStream_t> stream;   // one per shard, on its device: the shard's searches
    // a finished shard's list leaves on a stream of its own: with two searches in flight the shard's search stream already holds the NEXT
    // search's launches, and a copy enqueued behind them would hold this search's merge back by a whole batch
    std::vector<hipStream_t> copy_stream;
    hipStream_t merge_stream = nullptr;  // on devices[0]: merge + D2H of HOST-located searches (DEVICE-located ones merge on the caller's stream)
    NodeSlot slot[2];
    int next_slot = 0, n_pending = 0;  // FIFO: the oldest pending search sits in slot (next_slot - n_pending) & 1
    int last_finished = 0;             // the slot whose profile events `get_stat` reads
    bool finishing = false;            // a `search_finish` is running (outside the mutex: it waits for the devices) on the oldest slot
    const int32_t* q_labels = nullptr;  // the caller's per-query labels for the next searches (host, or devices[0])
    int q_labels_per_query = 0, q_labels_location = VODHIP_HOST;
    bool has_row_labels = false;
    int64_t update_unrouted = 0;             // slots of the last update_rows that no shard owns (id < 0 or >= ntotal): skipped here
    int64_t remove_unrouted = 0;             // the same of the last remove_rows
    int64_t value_rows = 0, value_cols = 0;  // the value table of the posterior read-out as it was set (0, 0: none); the shards hold its rows
    // topology (read once at create): can devices[0] and shard g's device copy into each other's memory directly?  A shard without
    // peer access - or every shard but the first with `host_staging` set (bring-up, tests on a 1-GPU box) - exchanges its queries and
    // its top-k list with devices[0] through pinned host memory instead (two DMA hops over PCIe, no xGMI)
    std::vector<int> peer_ok;          // 2 = same device as devices[0], 1 = peer access both ways, 0 = none
    int64_t host_staging = 0;
    // add / reset / label changes / searches on one handle are serialised (the staging buffers and the shards' FIFOs are shared); a
    // `set_query_labels` + `search` pair is two calls: callers that filter from several threads go through a vodhip_batcher
    // param "profile" = 1: HIP events bracket the merge (recorded once every shard's list has arrived on devices[0]) and every shard's
    // copy of its list towards devices[0] - `vodhip_node_index_get_stat` reads them: "last_merge_ns", "last_copy_ns_max"
    int64_t profile = 0;
    std::mutex mu;
    bool staged(int g) const { return g > 0 && (host_staging != 0 || (device[g] != device[0] && peer_ok[g] == 0)); }
};

namespace {

int ensure(void** p, size_t* have, size_t want, size_t elem) {
    if (*have >= want && *p) return 0;
    if (*p) NODE_HIP_OK(hipFree(*p));
    *p = nullptr;
    *have = 0;
    const size_t n = want + want / 4 + 64;  // a little headroom: batch sizes wobble
    NODE_HIP_OK(hipMalloc(p, n * elem));
    *have = n;
    return 0;
}

// ---- what the host-synchronous calls (every operation but `search`) share ----------------------------------------------------------

// a message of log_partition_args_error (or of a check built on it), as the node calls report it: partition_args_fail of vodhip_api.hip
int node_partition_args_fail(const char* msg, int q_dtype, float beta) {
    if (!strcmp(msg, "invalid q_dtype")) return nfail("invalid q_dtype %d", q_dtype);
    if (!strncmp(msg, "beta", 4)) return nfail("beta=%g: %s", (double)beta, msg);
    return nfail("%s", msg);
}

// the index kinds no whole-store scan accepts; `what` names the operation in the message (scan_refusal of vodhip_api.hip)
int node_scan_refusal(const vodhip_node_index* nx, const char* what) {
    if (nx->dtype & VODHIP_L2) return nfail(vodhip::SCAN_REFUSES_L2, what);
    if (nx->dtype & VODHIP_EXACT_F32) return nfail(vodhip::SCAN_REFUSES_EXACT_F32, what);
    return 0;
}

// subset labels without row labels; the caller holds nx->mu
int node_labels_refusal(const vodhip_node_index* nx, const void* q_labels) {
    if (!q_labels || nx->has_row_labels) return 0;
    return nfail("set the row labels first (vodhip_node_index_set_row_labels)");
}

inline size_t query_bytes(const vodhip_node_index* nx, int64_t nq, int q_dtype) { return (size_t)nq * (size_t)nx->dim * elem_bytes(q_dtype); }
inline size_t label_bytes(const void* q_labels, int64_t nq, int n_per_query) { return q_labels ? (size_t)nq * (size_t)n_per_query * sizeof(int32_t) : 0; }

// The route of those calls: host inputs are replicated to every shard, every shard runs the flat call on its own device and stream,
// the per-shard outputs return through host memory (the caller folds them).  A SLOT is one stream-ordered device block per shard:
// an input is uploaded before the flat call, an output downloaded after it returned 0 - shard g's bytes land at base + g * bytes.
// A slot of no bytes (a NULL host pointer) allocates nothing and stays NULL.  The caller holds nx->mu.
struct ShardFanout {
    static constexpr int MAX_SLOTS = 9;  // (the key gradient)
    struct Slot { const void* up; char* down; size_t bytes; };
    vodhip_node_index* nx;
    Slot slot[MAX_SLOTS];
    int n_slots = 0;
    explicit ShardFanout(vodhip_node_index* nx_) : nx(nx_) {}
    int input(const void* host, size_t bytes) { return add({host, nullptr, host ? bytes : 0}); }
    int output(void* host_base, size_t bytes_per_shard) { return add({nullptr, (char*)host_base, host_base ? bytes_per_shard : 0}); }
    int add(Slot s) {
        assert(n_slots < MAX_SLOTS);
        slot[n_slots] = s;
        return n_slots++;
    }
    // call(g, p, stream): the flat call of shard g, p[i] = slot i on its device; 0, or -1 with vodhip_last_error() set.  Nothing is
    // waited for until every shard is enqueued (unless the flat call itself waits); the first error wins and ends the enqueueing
    template <class Call>
    int run(Call&& call) {
        const int G = nx->n;
        std::vector<void*> dev((size_t)G * MAX_SLOTS, nullptr);
        bool failed = false;
        std::string err;
        auto hip_step = [&](hipError_t e, const char* what) {
            if (e != hipSuccess && !failed) {
                (void)hipGetLastError();
                err = std::string(what) + " failed: " + hipGetErrorString(e);
                failed = true;
            }
            return e == hipSuccess;
        };
        auto enqueue = [&](int g) {
            hipStream_t st = nx->stream[g];
            void** p = &dev[(size_t)g * MAX_SLOTS];
            if (!hip_step(hipSetDevice(nx->device[g]), "hipSetDevice")) return;
            for (int i = 0; i < n_slots; ++i)
                if (slot[i].bytes && !hip_step(hipMallocAsync(&p[i], slot[i].bytes, st), "hipMallocAsync")) return;
            for (int i = 0; i < n_slots; ++i)
                if (slot[i].bytes && slot[i].up && !hip_step(hipMemcpyAsync(p[i], slot[i].up, slot[i].bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync")) return;
            if (call(g, (void* const*)p, st)) {
                err = std::string("shard ") + std::to_string(g) + ": " + vodhip_last_error();
                failed = true;
                return;
            }
            for (int i = 0; i < n_slots; ++i)
                if (slot[i].bytes && slot[i].down)
                    hip_step(hipMemcpyAsync(slot[i].down + (size_t)g * slot[i].bytes, p[i], slot[i].bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
        };
        for (int g = 0; g < G && !failed; ++g) enqueue(g);
        for (int g = 0; g < G; ++g) {  // (also after a failure: what was enqueued reads and writes the caller's host memory)
            if (hipSetDevice(nx->device[g]) != hipSuccess) continue;
            for (int i = 0; i < MAX_SLOTS; ++i)
                if (void* p = dev[(size_t)g * MAX_SLOTS + i]) (void)hipFreeAsync(p, nx->stream[g]);
            hip_step(hipStreamSynchronize(nx->stream[g]), "hipStreamSynchronize");
        }
        (void)hipSetDevice(nx->device[0]);
        return failed ? nfail("%s", err.c_str()) : 0;
    }
};

}  // namespace

extern "C" {

int vodhip_node_index_create(int n_devices, const int* devices, int64_t dim, int store_dtype, int64_t capacity_rows,
                             vodhip_node_index_t** out) {
    if (!out) return nfail("out is NULL");
    if (n_devices < 1 || n_devices > 64 || !devices) return nfail("n_devices=%d out of range [1, 64]", n_devices);
    if (capacity_rows < 0) return nfail("invalid capacity=%lld", (long long)capacity_rows);
    if (store_dtype & VODHIP_L2) return nfail("VODHIP_L2 is not supported by the node index: the merge of the shards' lists orders by inner product (DESIGN.md 8)");
    vodhip_node_index* nx = new vodhip_node_index();
    nx->n = n_devices;
    nx->dim = dim;
    nx->dtype = store_dtype;
    nx->capacity = capacity_rows;
    nx->rows_per_shard = (capacity_rows + n_devices - 1) / n_devices;
    nx->device.assign(devices, devices + n_devices);
    nx->shard.assign(n_devices, nullptr);
    nx->stream.assign(n_devices, nullptr);
    nx->copy_stream.assign(n_devices, nullptr);
    for (NodeSlot& S : nx->slot) {
        S.arrived.assign(n_devices, nullptr);
        S.buf.resize(n_devices);
        S.pin_res.assign(n_devices, nullptr);
        S.pin_res_elems.assign(n_devices, 0);
        S.on_host.assign(n_devices, nullptr);
    }
    nx->peer_ok.assign(n_devices, 2);
    auto bail = [&](int rc) {
        const std::string keep = vodhip_last_error();
        vodhip_node_index_destroy(nx);
        vodhip::set_last_error(keep.c_str());
        return rc;
    };
    for (int g = 0; g < n_devices; ++g) {
        const int64_t lo = std::min(capacity_rows, g * nx->rows_per_shard), hi = std::min(capacity_rows, lo + nx->rows_per_shard);
        if (vodhip_index_create(devices[g], dim, store_dtype, hi - lo, &nx->shard[g])) return bail(-1);
        hipError_t e = hipSetDevice(devices[g]);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&nx->stream[g], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&nx->copy_stream[g], hipStreamNonBlocking);
        for (NodeSlot& S : nx->slot)
            if (e == hipSuccess) e = hipEventCreateWithFlags(&S.arrived[g], hipEventDisableTiming);
        if (e != hipSuccess) return bail(nfail("stream / event creation on device %d failed: %s", devices[g], hipGetErrorString(e)));
    }
    hipError_t e = hipSetDevice(devices[0]);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&nx->merge_stream, hipStreamNonBlocking);
    for (NodeSlot& S : nx->slot) {
        if (e == hipSuccess) e = hipEventCreateWithFlags(&S.ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&S.q_on_host, hipEventDisableTiming);
    }
    if (e != hipSuccess) return bail(nfail("event creation failed: %s", hipGetErrorString(e)));
    // topology: direct peer copies where both directions are possible (enabled here; "already enabled" is fine), host staging elsewhere
    for (int g = 0; g < n_devices; ++g) {
        if (devices[g] == devices[0]) continue;
        int to = 0, from = 0;
        if (hipDeviceCanAccessPeer(&to, devices[0], devices[g]) != hipSuccess) to = 0;
        if (hipDeviceCanAccessPeer(&from, devices[g], devices[0]) != hipSuccess) from = 0;
        nx->peer_ok[g] = (to && from) ? 1 : 0;
        if (nx->peer_ok[g]) {
            (void)hipSetDevice(devices[0]);
            hipError_t pe = hipDeviceEnablePeerAccess(devices[g], 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) nx->peer_ok[g] = 0;
            (void)hipSetDevice(devices[g]);
            pe = hipDeviceEnablePeerAccess(devices[0], 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) nx->peer_ok[g] = 0;
            (void)hipGetLastError();
        }
        if (nx->peer_ok[g]) {
            // the runtime said yes: prove it with a 256-byte round trip devices[0] -> devices[g] -> devices[0] before any search depends
            // on it (a node whose fabric is half configured answers "can access" and then fails the copy: host staging still works)
            void *a = nullptr, *b2 = nullptr;
            unsigned char probe[256], back[256];
            for (int i = 0; i < 256; ++i) probe[i] = (unsigned char)(i * 7 + g);
            memset(back, 0, sizeof(back));
            hipError_t pe = hipSetDevice(devices[0]);
            if (pe == hipSuccess) pe = hipMalloc(&a, 512);
            if (pe == hipSuccess) pe = hipSetDevice(devices[g]);
            if (pe == hipSuccess) pe = hipMalloc(&b2, 256);
            if (pe == hipSuccess) pe = hipSetDevice(devices[0]);
            if (pe == hipSuccess) pe = hipMemcpy(a, probe, 256, hipMemcpyHostToDevice);
            if (pe == hipSuccess) pe = hipMemcpyPeerAsync(b2, devices[g], a, devices[0], 256, nx->stream[0]);
            if (pe == hipSuccess) pe = hipStreamSynchronize(nx->stream[0]);
            if (pe == hipSuccess) pe = hipSetDevice(devices[g]);
            if (pe == hipSuccess) pe = hipMemcpyPeerAsync((char*)a + 256, devices[0], b2, devices[g], 256, nx->stream[g]);
            if (pe == hipSuccess) pe = hipStreamSynchronize(nx->stream[g]);
            if (pe == hipSuccess) pe = hipSetDevice(devices[0]);
            if (pe == hipSuccess) pe = hipMemcpy(back, (char*)a + 256, 256, hipMemcpyDeviceToHost);
            if (pe != hipSuccess || memcmp(probe, back, 256) != 0) nx->peer_ok[g] = 0;
            (void)hipSetDevice(devices[0]);
            if (a) (void)hipFree(a);
            (void)hipSetDevice(devices[g]);
            if (b2) (void)hipFree(b2);
            (void)hipGetLastError();
        }
    }
    (void)hipSetDevice(devices[0]);
    *out = nx;
    return 0;
}

int vodhip_node_index_peer_access(const vodhip_node_index_t* nx, int* out, int n) {
    if (!nx || !out || n < nx->n) return nfail("invalid arguments");
    for (int g = 0; g < nx->n; ++g) out[g] = nx->staged(g) ? 0 : nx->peer_ok[g];
    return nx->n;
}

int vodhip_node_index_destroy(vodhip_node_index_t* nx) {
    if (!nx) return 0;
    for (int g = 0; g < nx->n; ++g) {
        if (!nx->shard[g]) continue;  // create() failed before this shard existed: its device may not exist either
        (void)hipSetDevice(nx->device[g]);
        if (nx->stream[g]) (void)hipStreamSynchronize(nx->stream[g]);
        if (nx->shard[g]) (void)vodhip_index_destroy(nx->shard[g]);
        for (NodeSlot& S : nx->slot) {
            (void)hipFree(S.buf[g].q);
            (void)hipFree(S.buf[g].scores);
            (void)hipFree(S.buf[g].ids);
            (void)hipFree(S.buf[g].q_labels);
            if (S.arrived[g]) (void)hipEventDestroy(S.arrived[g]);
            if (S.on_host[g]) (void)hipEventDestroy(S.on_host[g]);
            if (S.pin_res[g]) (void)hipHostFree(S.pin_res[g]);
        }
        if (nx->copy_stream[g]) {
            (void)hipStreamSynchronize(nx->copy_stream[g]);
            (void)hipStreamDestroy(nx->copy_stream[g]);
        }
        if (nx->stream[g]) (void)hipStreamDestroy(nx->stream[g]);
    }
    if (nx->n && nx->shard[0]) (void)hipSetDevice(nx->device[0]);
    if (nx->merge_stream) {
        (void)hipStreamSynchronize(nx->merge_stream);
        (void)hipStreamDestroy(nx->merge_stream);
    }
    for (NodeSlot& S : nx->slot) {
        if (S.pin_q) (void)hipHostFree(S.pin_q);
        if (S.q_on_host) (void)hipEventDestroy(S.q_on_host);
        for (hipEvent_t e : S.copy_ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : S.merge_ev)
            if (e) (void)hipEventDestroy(e);
        (void)hipFree(S.gathered_scores);
        (void)hipFree(S.gathered_ids);
        (void)hipFree(S.merged_scores);
        (void)hipFree(S.merged_ids);
        if (S.ready) (void)hipEventDestroy(S.ready);
    }
    delete nx;
    (void)hipGetLastError();  // best-effort teardown: nothing of it may resurface in the caller's next launch check
    return 0;
}

int vodhip_node_index_add(vodhip_node_index_t* nx, const void* rows, int64_t n_rows, int src_dtype) {
    if (!nx) return nfail("index is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (n_rows < 0 || (n_rows > 0 && !rows)) return nfail("invalid rows");
    if (src_dtype < 0 || src_dtype > 2) return nfail("invalid src_dtype %d", src_dtype);
    if (nx->n_pending) return nfail("%d searches are in flight: finish them before adding rows", nx->n_pending);
    if (nx->ntotal + n_rows > nx->capacity)
        return nfail("index full: ntotal=%lld + %lld > capacity=%lld", (long long)nx->ntotal, (long long)n_rows, (long long)nx->capacity);
    // global rows [ntotal, ntotal + n_rows): the part inside shard g's range goes to shard g; the shards ingest concurrently
    // (one host thread each: every device has its own DMA engines and PCIe link)
    struct Part { int g; int64_t first, count; };
    std::vector<Part> parts;
    for (int g = 0; g < nx->n; ++g) {
        const int64_t lo = g * nx->rows_per_shard, hi = lo + nx->rows_per_shard;
        const int64_t a = std::max(lo, nx->ntotal), b = std::min(hi, nx->ntotal + n_rows);
        if (b > a) parts.push_back({g, a - nx->ntotal, b - a});
    }
    std::vector<std::string> errors(parts.size());
    std::vector<int> rcs(parts.size(), 0);
    auto work = [&](size_t i) {
        const Part& p = parts[i];
        const char* src = (const char*)rows + (size_t)p.first * (size_t)nx->dim * elem_bytes(src_dtype);
        rcs[i] = vodhip_index_add(nx->shard[p.g], src, p.count, src_dtype, VODHIP_HOST, nx->stream[p.g]);
        if (rcs[i]) errors[i] = vodhip_last_error();  // thread-local text: carried back to the caller's thread
    };
    if (parts.size() == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (size_t i = 0; i < parts.size(); ++i) pool.emplace_back(work, i);
        for (auto& t : pool) t.join();
    }
    for (size_t i = 0; i < parts.size(); ++i)
        if (rcs[i]) return nfail("shard %d: %s", parts[i].g, errors[i].c_str());
    nx->ntotal += n_rows;
    return 0;
}

// H2u behind the one handle: routed on the host (update_fold.h) - shard g gets its own slots and rows, nothing is replicated
int vodhip_node_index_update_rows(vodhip_node_index_t* nx, const int64_t* ids, int64_t row_begin, const void* rows, int64_t n, int src_dtype, int mode,
                                  float alpha) {
    if (!nx) return nfail("index is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (const char* msg = vodhip::update_rows_args_error(ids != nullptr, row_begin, rows, n, src_dtype, VODHIP_HOST, mode, alpha, nx->ntotal)) {
        if (!strcmp(msg, "invalid src_dtype")) return nfail("invalid src_dtype %d", src_dtype);
        if (!strcmp(msg, "invalid mode")) return nfail("invalid mode %d", mode);
        if (!strncmp(msg, "alpha", 5)) return nfail("alpha=%g: %s", (double)alpha, msg);
        if (!strncmp(msg, "row range", 9)) return nfail("rows [%lld, %lld + %lld), ntotal=%lld: %s", (long long)row_begin, (long long)row_begin, (long long)n, (long long)nx->ntotal, msg);
        return nfail("n=%lld: %s", (long long)n, msg);
    }
    if (nx->n_pending) return nfail("%d searches are in flight: finish them before updating rows", nx->n_pending);
    const size_t row_bytes = (size_t)nx->dim * elem_bytes(src_dtype);
    vodhip::UpdateRoute route;
    if (ids) route = vodhip::route_update_slots(ids, n, nx->rows_per_shard, nx->n, nx->ntotal);
    nx->update_unrouted = route.skipped;
    std::vector<int64_t> shard_ids;
    std::vector<char> shard_rows;
    // (a shard without a slot still takes the call, with n = 0: its stats of an earlier call must not enter this call's sums)
    for (int g = 0; g < nx->n; ++g) {
        const int64_t base = g * nx->rows_per_shard;
        int rc;
        if (!ids) {
            int64_t lo, hi;
            vodhip::split_update_range(row_begin, n, nx->rows_per_shard, g, &lo, &hi);
            rc = vodhip_index_update_rows(nx->shard[g], nullptr, hi > lo ? row_begin + lo - base : 0, (const char*)rows + (size_t)lo * row_bytes, hi - lo, src_dtype,
                                          VODHIP_HOST, mode, alpha, 0, nx->stream[g]);
        } else {
            const int64_t first = route.first[(size_t)g], cnt = route.first[(size_t)g + 1] - first;
            shard_ids.resize((size_t)cnt);
            shard_rows.resize((size_t)cnt * row_bytes);
            for (int64_t i = 0; i < cnt; ++i) {
                const int64_t j = route.slot[(size_t)(first + i)];
                shard_ids[(size_t)i] = ids[j];
                memcpy(shard_rows.data() + (size_t)i * row_bytes, (const char*)rows + (size_t)j * row_bytes, row_bytes);
            }
            rc = vodhip_index_update_rows(nx->shard[g], cnt ? shard_ids.data() : nullptr, 0, cnt ? shard_rows.data() : nullptr, cnt, src_dtype, VODHIP_HOST, mode,
                                          alpha, base, nx->stream[g]);
        }
        if (rc) return nfail("shard %d: %s", g, std::string(vodhip_last_error()).c_str());
    }
    return 0;
}

// H2r behind the one handle: the slots routed as for H2u, every shard compacted by the flat call, then the survivors moved between the
// shards until the layout is the one `add` fills (remove_fold.h: plan_remove_segments)
int vodhip_node_index_remove_rows(vodhip_node_index_t* nx, const int64_t* ids, int64_t row_begin, int64_t n, int64_t* new_ids, int64_t* n_removed) {
    if (!nx) return nfail("index is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (const char* msg = vodhip::remove_rows_args_error(ids != nullptr, row_begin, n, VODHIP_HOST, nx->ntotal)) {
        if (!strncmp(msg, "row range", 9)) return nfail("rows [%lld, %lld + %lld), ntotal=%lld: %s", (long long)row_begin, (long long)row_begin, (long long)n, (long long)nx->ntotal, msg);
        return nfail("n=%lld: %s", (long long)n, msg);
    }
    if (nx->n_pending) return nfail("%d searches are in flight: finish them before removing rows", nx->n_pending);
    if (nx->value_cols && nx->value_rows != nx->ntotal)  // (before any shard compacts: the flat call would refuse on the short shard only)
        return nfail("remove_rows: the value table holds %lld rows, the index %lld: set the table again (or clear it) after adding rows, then remove",
                     (long long)nx->value_rows, (long long)nx->ntotal);
    const int G = nx->n;
    vodhip::UpdateRoute route;
    if (ids) route = vodhip::route_update_slots(ids, n, nx->rows_per_shard, G, nx->ntotal);
    nx->remove_unrouted = route.skipped;
    std::vector<int64_t> old_rows((size_t)G), keep((size_t)G), shard_ids;
    std::vector<std::vector<int64_t>> local_map((size_t)(new_ids ? G : 0));
    auto restore = [&](int rc) {
        (void)hipSetDevice(nx->device[0]);
        return rc;
    };
    // (a shard without a slot still takes the call, with n = 0: its stats of an earlier call must not enter this call's sums)
    for (int g = 0; g < G; ++g) {
        const int64_t base = g * nx->rows_per_shard;
        if (vodhip_index_ntotal(nx->shard[g], &old_rows[(size_t)g])) return restore(-1);
        int64_t* map_dev = nullptr;
        int64_t cnt = 0;
        if (new_ids && old_rows[(size_t)g] > 0) {
            NODE_HIP_OK(hipSetDevice(nx->device[g]));
            NODE_HIP_OK(hipMalloc((void**)&map_dev, (size_t)old_rows[(size_t)g] * sizeof(int64_t)));
        }
        int rc;
        if (!ids) {
            int64_t lo, hi;
            vodhip::split_remove_range(row_begin, n, nx->rows_per_shard, g, &lo, &hi);
            cnt = hi - lo;
            rc = vodhip_index_remove_rows(nx->shard[g], nullptr, lo, cnt, VODHIP_HOST, 0, map_dev, nullptr, nx->stream[g]);
        } else {
            const int64_t first = route.first[(size_t)g];
            cnt = route.first[(size_t)g + 1] - first;
            shard_ids.resize((size_t)cnt);
            for (int64_t i = 0; i < cnt; ++i) shard_ids[(size_t)i] = ids[route.slot[(size_t)(first + i)]];
            rc = vodhip_index_remove_rows(nx->shard[g], cnt ? shard_ids.data() : nullptr, 0, cnt, VODHIP_HOST, base, map_dev, nullptr, nx->stream[g]);
        }
        std::string err = rc ? std::string(vodhip_last_error()) : std::string();
        if (map_dev) {
            local_map[(size_t)g].resize((size_t)old_rows[(size_t)g]);
            hipError_t e = hipSetDevice(nx->device[g]);
            if (rc == 0 && cnt == 0) {  // (the flat call writes no map for an empty call: the identity)
                for (int64_t r = 0; r < old_rows[(size_t)g]; ++r) local_map[(size_t)g][(size_t)r] = r;
            } else if (rc == 0) {
                if (e == hipSuccess) e = hipMemcpyAsync(local_map[(size_t)g].data(), map_dev, (size_t)old_rows[(size_t)g] * sizeof(int64_t), hipMemcpyDeviceToHost, nx->stream[g]);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(nx->stream[g]);
            (void)hipFree(map_dev);
            if (rc == 0 && e != hipSuccess) {
                (void)hipGetLastError();
                return restore(nfail("shard %d: reading the id map failed: %s", g, hipGetErrorString(e)));
            }
        }
        if (rc) return restore(nfail("shard %d: %s", g, err.c_str()));
        if (vodhip_index_ntotal(nx->shard[g], &keep[(size_t)g])) return restore(-1);
    }
    // every shard holds its survivors in rows [0, keep[g]): move them to where `add` would have put them, one segment after the other
    const vodhip::RemoveSegmentPlan plan = vodhip::plan_remove_segments(keep.data(), G, nx->rows_per_shard);
    for (int g = 0; g < G; ++g) {  // (a shard's own compaction is only enqueued, and a segment reads another shard's rows)
        NODE_HIP_OK(hipSetDevice(nx->device[g]));
        NODE_HIP_OK(hipStreamSynchronize(nx->stream[g]));
    }
    for (const vodhip::RemoveSegment& s : plan.segments) {
        if (vodhip::index_remove_move_rows(nx->shard[(size_t)s.src_shard], s.src_row, nx->shard[(size_t)s.dst_shard], s.dst_row, s.n, nx->stream[(size_t)s.dst_shard]))
            return restore(nfail("moving rows from shard %d to shard %d: %s", s.src_shard, s.dst_shard, std::string(vodhip_last_error()).c_str()));
    }
    int64_t total = 0;
    for (int g = 0; g < G; ++g) {
        if (plan.ntotal[(size_t)g] != keep[(size_t)g] || !plan.segments.empty()) {
            if (vodhip::index_remove_set_ntotal(nx->shard[g], plan.ntotal[(size_t)g], nx->stream[g]))
                return restore(nfail("shard %d: %s", g, std::string(vodhip_last_error()).c_str()));
        }
        total += plan.ntotal[(size_t)g];
    }
    if (new_ids) {
        int64_t before = 0;  // survivors of the shards below
        for (int g = 0; g < G; ++g) {
            int64_t* out = new_ids + g * nx->rows_per_shard;
            for (int64_t r = 0; r < old_rows[(size_t)g]; ++r) {
                const int64_t v = local_map[(size_t)g].empty() ? -1 : local_map[(size_t)g][(size_t)r];
                out[r] = v < 0 ? -1 : before + v;
            }
            before += keep[(size_t)g];
        }
    }
    if (n_removed) *n_removed = nx->ntotal - total;
    if (nx->value_cols) nx->value_rows = total;
    nx->ntotal = total;
    return restore(0);
}

int vodhip_node_index_reset(vodhip_node_index_t* nx) {
    if (!nx) return nfail("index is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (nx->n_pending) return nfail("%d searches are in flight: finish them before resetting the index", nx->n_pending);
    for (int g = 0; g < nx->n; ++g)
        if (vodhip_index_reset(nx->shard[g])) return -1;
    nx->ntotal = 0;
    nx->value_rows = nx->value_cols = 0;  // (every shard dropped its part of the value table)
    return 0;
}

int vodhip_node_index_ntotal(const vodhip_node_index_t* nx, int64_t* out) {
    if (!nx || !out) return nfail("NULL argument");
    *out = nx->ntotal;
    return 0;
}

int vodhip_node_index_n_shards(const vodhip_node_index_t* nx) { return nx ? nx->n : nfail("index is NULL"); }

int vodhip_node_index_shard(vodhip_node_index_t* nx, int g, vodhip_index_t** shard, int64_t* id_base, int* device) {
    if (!nx) return nfail("index is NULL");
    if (g < 0 || g >= nx->n) return nfail("shard %d out of range [0, %d)", g, nx->n);
    if (shard) *shard = nx->shard[g];
    if (id_base) *id_base = g * nx->rows_per_shard;
    if (device) *device = nx->device[g];
    return 0;
}

int vodhip_node_index_set_row_labels(vodhip_node_index_t* nx, const int32_t* labels, int64_t n_rows) {
    if (!nx) return nfail("index is NULL");
    if (labels && (n_rows < 0 || n_rows > nx->capacity)) return nfail("n_rows=%lld out of range", (long long)n_rows);
    std::lock_guard<std::mutex> guard(nx->mu);
    for (int g = 0; g < nx->n; ++g) {
        const int64_t lo = std::min<int64_t>(n_rows, g * nx->rows_per_shard), hi = std::min<int64_t>(n_rows, lo + nx->rows_per_shard);
        if (!labels) {
            if (vodhip_index_set_row_labels(nx->shard[g], nullptr, 0, VODHIP_HOST, nullptr)) return -1;
        } else if (vodhip_index_set_row_labels(nx->shard[g], labels + lo, hi - lo, VODHIP_HOST, nx->stream[g])) {
            return -1;
        }
    }
    nx->has_row_labels = labels != nullptr;
    if (!labels) nx->q_labels = nullptr;
    return 0;
}

// The value table of the posterior read-out behind the one handle: a HOST table for the global rows, split by shard row ranges
// (readout_fold.h).
int vodhip_node_index_set_row_values(vodhip_node_index_t* nx, const void* values, int64_t n_rows, int64_t n_cols, int src_dtype) {
    if (!nx) return nfail("index is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (nx->n_pending) return nfail("%d searches are in flight: finish them before changing the row values", nx->n_pending);
    if (values) {
        if (const char* msg = vodhip::row_values_args_error(n_rows, n_cols, src_dtype, VODHIP_HOST, nx->ntotal)) {
            if (!strcmp(msg, "invalid src_dtype")) return nfail("invalid src_dtype %d", src_dtype);
            if (msg[2] == 'c') return nfail("n_cols=%lld: %s (wider tables are not supported)", (long long)n_cols, msg);
            return nfail("n_rows=%lld, ntotal=%lld: %s", (long long)n_rows, (long long)nx->ntotal, msg);
        }
    }
    nx->value_rows = nx->value_cols = 0;
    for (int g = 0; g < nx->n; ++g) {
        int64_t lo = 0, hi = 0;
        if (values) vodhip::readout_shard_rows(n_rows, nx->rows_per_shard, g, &lo, &hi);
        if (!values) {
            if (vodhip_index_set_row_values(nx->shard[g], nullptr, 0, 0, 0, VODHIP_HOST, nx->stream[g])) return -1;
        } else {  // (a shard past the table's end holds no row: it gets a table of no rows and reads out the zero row)
            const char* src = (const char*)values + (size_t)lo * (size_t)n_cols * elem_bytes(src_dtype);
            if (vodhip_index_set_row_values(nx->shard[g], src, hi - lo, n_cols, src_dtype, VODHIP_HOST, nx->stream[g])) return -1;
        }
    }
    if (values) {
        nx->value_rows = n_rows;
        nx->value_cols = n_cols;
    }
    return 0;
}

int vodhip_node_index_row_values_info(const vodhip_node_index_t* nx, int64_t* n_rows, int64_t* n_cols) {
    if (!nx) return nfail("index is NULL");
    if (n_rows) *n_rows = nx->value_cols ? nx->value_rows : 0;
    if (n_cols) *n_cols = nx->value_cols;
    return 0;
}

int vodhip_node_index_set_query_labels(vodhip_node_index_t* nx, const int32_t* q_labels, int n_per_query, int location) {
    if (!nx) return nfail("index is NULL");
    if (q_labels && (n_per_query < 1 || n_per_query > 64)) return nfail("n_per_query must be in [1, 64]");
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (location != VODHIP_HOST && location != VODHIP_DEVICE) return nfail("invalid location %d", location);
    std::lock_guard<std::mutex> guard(nx->mu);
    nx->q_labels = q_labels;
    nx->q_labels_per_query = q_labels ? n_per_query : 0;
    nx->q_labels_location = location;
    return 0;
}

int vodhip_node_index_set_param(vodhip_node_index_t* nx, const char* key, int64_t value) {
    if (!nx) return nfail("index is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (key && !strcmp(key, "host_staging")) {  // 1: every shard but the first exchanges with devices[0] through pinned host memory
        nx->host_staging = value;
        return 0;
    }
    if (key && !strcmp(key, "profile")) nx->profile = value;  // (and on every shard: its filter launches are bracketed too)
    for (int g = 0; g < nx->n; ++g)
        if (vodhip_index_set_param(nx->shard[g], key, value)) return -1;
    return 0;
}

}  // extern "C"

namespace {

// step 1 of a search, into slot `S`: the query batch reaches every device (replicated: nq * dim * 2-4 bytes), then every shard's search is
// enqueued - nothing is waited for, so the devices run side by side and the call returns while they do
int node_enqueue_locked(vodhip_node_index* nx, NodeSlot& S, const void* queries, int q_dtype, int64_t nq, int k, int location,
                        float* out_scores, int64_t* out_ids, void* stream_) {
    const int G = nx->n, dev0 = nx->device[0];
    hipStream_t user = location == VODHIP_DEVICE ? (hipStream_t)stream_ : nx->merge_stream;
    const size_t q_bytes = (size_t)nq * (size_t)nx->dim * elem_bytes(q_dtype), res = (size_t)nq * (size_t)k;
    S.timed = false;
    if (nx->profile && S.copy_ev.empty()) {
        S.copy_ev.assign((size_t)2 * G, nullptr);
        for (int g = 0; g < G; ++g) {
            NODE_HIP_OK(hipSetDevice(nx->device[g]));
            NODE_HIP_OK(hipEventCreate(&S.copy_ev[2 * g]));
            NODE_HIP_OK(hipEventCreate(&S.copy_ev[2 * g + 1]));
        }
        NODE_HIP_OK(hipSetDevice(dev0));
        NODE_HIP_OK(hipEventCreate(&S.merge_ev[0]));
        NODE_HIP_OK(hipEventCreate(&S.merge_ev[1]));
    }
    // buffers (grown on demand, kept)
    for (int g = 0; g < G; ++g) {
        NODE_HIP_OK(hipSetDevice(nx->device[g]));
        ShardBuffers& b = S.buf[g];
        size_t rs = b.res_elems, ri = b.res_elems;
        if (ensure(&b.q, &b.q_bytes, q_bytes, 1)) return -1;
        if (ensure((void**)&b.scores, &rs, res, sizeof(float))) return -1;
        if (ensure((void**)&b.ids, &ri, res, sizeof(int64_t))) return -1;
        b.res_elems = std::min(rs, ri);
    }
    NODE_HIP_OK(hipSetDevice(dev0));
    if (G > 1) {
        size_t gs = S.gathered_elems, gi = S.gathered_elems;
        if (ensure((void**)&S.gathered_scores, &gs, res * G, sizeof(float))) return -1;
        if (ensure((void**)&S.gathered_ids, &gi, res * G, sizeof(int64_t))) return -1;
        S.gathered_elems = std::min(gs, gi);
    }
    if (location == VODHIP_HOST) {
        size_t ms = S.merged_elems, mi = S.merged_elems;
        if (ensure((void**)&S.merged_scores, &ms, res, sizeof(float))) return -1;
        if (ensure((void**)&S.merged_ids, &mi, res, sizeof(int64_t))) return -1;
        S.merged_elems = std::min(ms, mi);
    }
    float* final_scores = location == VODHIP_HOST ? S.merged_scores : out_scores;
    int64_t* final_ids = location == VODHIP_HOST ? S.merged_ids : out_ids;

    if (location == VODHIP_DEVICE) NODE_HIP_OK(hipEventRecord(S.ready, user));  // the caller's stream has produced the queries
    bool any_staged = false;
    for (int g = 0; g < G; ++g) any_staged = any_staged || nx->staged(g);
    const size_t lab_bytes = nx->q_labels ? (size_t)nq * (size_t)nx->q_labels_per_query * sizeof(int32_t) : 0;
    const bool stage_q = any_staged && location == VODHIP_DEVICE, stage_lab = any_staged && nx->q_labels && nx->q_labels_location == VODHIP_DEVICE;
    if (stage_q || stage_lab) {
        // shards without peer access read the batch from pinned host memory: ONE copy down from devices[0], then one copy up per shard
        const size_t want = q_bytes + lab_bytes + 64;
        if (S.pin_q_bytes < want) {
            if (S.pin_q) NODE_HIP_OK(hipHostFree(S.pin_q));
            S.pin_q = nullptr;
            NODE_HIP_OK(hipHostMalloc(&S.pin_q, want + want / 4, hipHostMallocDefault));
            S.pin_q_bytes = want + want / 4;
        }
        if (stage_q) NODE_HIP_OK(hipMemcpyAsync(S.pin_q, queries, q_bytes, hipMemcpyDeviceToHost, user));
        if (stage_lab) NODE_HIP_OK(hipMemcpyAsync((char*)S.pin_q + q_bytes, nx->q_labels, lab_bytes, hipMemcpyDeviceToHost, user));
        NODE_HIP_OK(hipEventRecord(S.q_on_host, user));
    }
    for (int g = 0; g < G; ++g) {
        NODE_HIP_OK(hipSetDevice(nx->device[g]));
        const bool staged = nx->staged(g);
        if (location == VODHIP_HOST) {
            NODE_HIP_OK(hipMemcpyAsync(S.buf[g].q, queries, q_bytes, hipMemcpyHostToDevice, nx->stream[g]));
        } else if (staged) {
            NODE_HIP_OK(hipStreamWaitEvent(nx->stream[g], S.q_on_host, 0));
            NODE_HIP_OK(hipMemcpyAsync(S.buf[g].q, S.pin_q, q_bytes, hipMemcpyHostToDevice, nx->stream[g]));
        } else {
            NODE_HIP_OK(hipStreamWaitEvent(nx->stream[g], S.ready, 0));
            if (nx->device[g] == dev0) NODE_HIP_OK(hipMemcpyAsync(S.buf[g].q, queries, q_bytes, hipMemcpyDeviceToDevice, nx->stream[g]));
            else NODE_HIP_OK(hipMemcpyPeerAsync(S.buf[g].q, nx->device[g], queries, dev0, q_bytes, nx->stream[g]));
        }
        if (nx->q_labels) {  // the batch's subset labels travel with the queries
            const size_t n_lab = (size_t)nq * (size_t)nx->q_labels_per_query;
            if (ensure((void**)&S.buf[g].q_labels, &S.buf[g].q_label_elems, n_lab, sizeof(int32_t))) return -1;
            if (nx->q_labels_location == VODHIP_HOST)
                NODE_HIP_OK(hipMemcpyAsync(S.buf[g].q_labels, nx->q_labels, n_lab * sizeof(int32_t), hipMemcpyHostToDevice, nx->stream[g]));
            else if (staged) {
                NODE_HIP_OK(hipStreamWaitEvent(nx->stream[g], S.q_on_host, 0));
                NODE_HIP_OK(hipMemcpyAsync(S.buf[g].q_labels, (char*)S.pin_q + q_bytes, n_lab * sizeof(int32_t), hipMemcpyHostToDevice, nx->stream[g]));
            } else if (nx->device[g] == dev0)
                NODE_HIP_OK(hipMemcpyAsync(S.buf[g].q_labels, nx->q_labels, n_lab * sizeof(int32_t), hipMemcpyDeviceToDevice, nx->stream[g]));
            else
                NODE_HIP_OK(hipMemcpyPeerAsync(S.buf[g].q_labels, nx->device[g], nx->q_labels, dev0, n_lab * sizeof(int32_t), nx->stream[g]));
            if (vodhip_index_set_query_labels(nx->shard[g], S.buf[g].q_labels, nx->q_labels_per_query)) return -1;
        } else if (nx->has_row_labels) {
            if (vodhip_index_set_query_labels(nx->shard[g], nullptr, 0)) return -1;
        }
        // a G = 1 index writes the caller's / the merged buffers directly
        float* s_out = G == 1 ? final_scores : S.buf[g].scores;
        int64_t* i_out = G == 1 ? final_ids : S.buf[g].ids;
        if (vodhip_index_search_async(nx->shard[g], S.buf[g].q, q_dtype, nq, k, g * nx->rows_per_shard, s_out, i_out, nx->stream[g])) {
            const std::string keep = vodhip_last_error();
            return nfail("shard %d: %s", g, keep.c_str());
        }
        S.enqueued[g] = 1;
    }
    NODE_HIP_OK(hipSetDevice(dev0));
    S.nq = nq;
    S.k = k;
    S.location = location;
    S.out_scores = out_scores;
    S.out_ids = out_ids;
    S.user = user;
    return 0;
}

// steps 2 and 3 of the search in slot `S`: the exactness check of every shard (host side; a shard that needs a recovery pass runs it on its
// own stream), its list travels to devices[0], the merge there
int node_finish_locked(vodhip_node_index* nx, NodeSlot& S) {
    const int G = nx->n, dev0 = nx->device[0];
    const int64_t nq = S.nq;
    const int k = S.k, location = S.location;
    hipStream_t user = S.user;
    const size_t res = (size_t)nq * (size_t)k;
    float* final_scores = location == VODHIP_HOST ? S.merged_scores : S.out_scores;
    int64_t* final_ids = location == VODHIP_HOST ? S.merged_ids : S.out_ids;
    int rc = 0;
    std::string first_error;
    for (int g = 0; g < G; ++g) {
        S.enqueued[g] = 0;
        if (vodhip_index_search_finish(nx->shard[g], nx->stream[g])) {
            if (!rc) first_error = std::string("shard ") + std::to_string(g) + ": " + vodhip_last_error();
            rc = -1;
            continue;
        }
        if (G == 1 || rc) continue;
        NODE_HIP_OK(hipSetDevice(nx->device[g]));
        float* ds = S.gathered_scores + (size_t)g * res;
        int64_t* di = S.gathered_ids + (size_t)g * res;
        hipStream_t cs = nx->copy_stream[g];  // (the shard's search is complete - `finish` waited for it on the host - so the copy depends on nothing)
        if (nx->staged(g)) {
            // no peer access: the list goes down to pinned host memory on the shard's copy stream and up to devices[0] on the merge stream
            if (S.pin_res_elems[g] < res) {
                if (S.pin_res[g]) NODE_HIP_OK(hipHostFree(S.pin_res[g]));
                S.pin_res[g] = nullptr;
                NODE_HIP_OK(hipHostMalloc(&S.pin_res[g], (res + res / 4 + 64) * 12, hipHostMallocDefault));
                S.pin_res_elems[g] = res + res / 4 + 64;
            }
            if (!S.on_host[g]) NODE_HIP_OK(hipEventCreateWithFlags(&S.on_host[g], hipEventDisableTiming));
            char* pin = (char*)S.pin_res[g];
            if (nx->profile) NODE_HIP_OK(hipEventRecord(S.copy_ev[2 * g], cs));
            NODE_HIP_OK(hipMemcpyAsync(pin, S.buf[g].scores, res * sizeof(float), hipMemcpyDeviceToHost, cs));
            NODE_HIP_OK(hipMemcpyAsync(pin + S.pin_res_elems[g] * 4, S.buf[g].ids, res * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
            if (nx->profile) NODE_HIP_OK(hipEventRecord(S.copy_ev[2 * g + 1], cs));  // (the down-leg; the up-leg runs on the merge stream)
            NODE_HIP_OK(hipEventRecord(S.on_host[g], cs));
            NODE_HIP_OK(hipSetDevice(dev0));
            NODE_HIP_OK(hipStreamWaitEvent(user, S.on_host[g], 0));
            NODE_HIP_OK(hipMemcpyAsync(ds, pin, res * sizeof(float), hipMemcpyHostToDevice, user));
            NODE_HIP_OK(hipMemcpyAsync(di, pin + S.pin_res_elems[g] * 4, res * sizeof(int64_t), hipMemcpyHostToDevice, user));
            NODE_HIP_OK(hipEventRecord(S.arrived[g], user));  // (the merge below runs on `user` anyway: this keeps the wait list uniform)
            continue;
        }
        if (nx->profile) NODE_HIP_OK(hipEventRecord(S.copy_ev[2 * g], cs));
        if (nx->device[g] == dev0) {
            NODE_HIP_OK(hipMemcpyAsync(ds, S.buf[g].scores, res * sizeof(float), hipMemcpyDeviceToDevice, cs));
            NODE_HIP_OK(hipMemcpyAsync(di, S.buf[g].ids, res * sizeof(int64_t), hipMemcpyDeviceToDevice, cs));
        } else {
            NODE_HIP_OK(hipMemcpyPeerAsync(ds, dev0, S.buf[g].scores, nx->device[g], res * sizeof(float), cs));
            NODE_HIP_OK(hipMemcpyPeerAsync(di, dev0, S.buf[g].ids, nx->device[g], res * sizeof(int64_t), cs));
        }
        if (nx->profile) NODE_HIP_OK(hipEventRecord(S.copy_ev[2 * g + 1], cs));
        NODE_HIP_OK(hipEventRecord(S.arrived[g], cs));
    }
    if (rc) return nfail("%s", first_error.c_str());
    // the merge on devices[0], on the caller's stream (DEVICE) or shard 0's (HOST)
    NODE_HIP_OK(hipSetDevice(dev0));
    if (G > 1) {
        for (int g = 0; g < G; ++g) NODE_HIP_OK(hipStreamWaitEvent(user, S.arrived[g], 0));
        if (nx->profile) NODE_HIP_OK(hipEventRecord(S.merge_ev[0], user));  // every list has arrived: what follows is the merge alone
        if (vodhip_merge_topk(S.gathered_scores, S.gathered_ids, G, nq, k, k, final_scores, final_ids, user)) return -1;
        if (nx->profile) NODE_HIP_OK(hipEventRecord(S.merge_ev[1], user));
        S.timed = nx->profile != 0;
    }
    // (G == 1: the one shard wrote the final buffers itself and its search is complete - nothing to order on the device)
    if (location == VODHIP_HOST) {
        NODE_HIP_OK(hipMemcpyAsync(S.out_scores, final_scores, res * sizeof(float), hipMemcpyDeviceToHost, user));
        NODE_HIP_OK(hipMemcpyAsync(S.out_ids, final_ids, res * sizeof(int64_t), hipMemcpyDeviceToHost, user));
        NODE_HIP_OK(hipStreamSynchronize(user));
    }
    if (location == VODHIP_DEVICE) {
        // the slot's NEXT search must not refill `gathered` / the shard buffers before this merge has read them: every shard stream waits
        // for `ready`, recorded here behind the merge (the other slot's search - already enqueued on the shard streams - is ahead of the wait)
        NODE_HIP_OK(hipEventRecord(S.ready, user));
        for (int g = 0; g < G; ++g) {
            NODE_HIP_OK(hipSetDevice(nx->device[g]));
            NODE_HIP_OK(hipStreamWaitEvent(nx->stream[g], S.ready, 0));
        }
        NODE_HIP_OK(hipSetDevice(dev0));
    }
    return 0;
}

int node_check_args(vodhip_node_index* nx, const void* queries, int q_dtype, int64_t nq, int k, int location, float* out_scores, int64_t* out_ids) {
    if (k < 1 || k > VODHIP_MAX_K) return nfail("k=%d out of range [1, %d]", k, VODHIP_MAX_K);
    if (nq < 0 || (nq > 0 && (!queries || !out_scores || !out_ids))) return nfail("invalid query / output pointers");
    if (q_dtype < 0 || q_dtype > 2) return nfail("invalid q_dtype %d", q_dtype);
    if (location != VODHIP_HOST && location != VODHIP_DEVICE) return nfail("invalid location %d", location);
    (void)nx;
    return 0;
}

// whatever failed (a copy, an allocation, one shard's search): no shard keeps a search of the failed call in its FIFO - the next call's
// `finish` must meet the next call's search
void node_drain_failed(vodhip_node_index* nx, NodeSlot& S) {
    const std::string keep = vodhip_last_error();
    for (int g = 0; g < nx->n; ++g)
        if (S.enqueued[(size_t)g]) (void)vodhip_index_search_finish(nx->shard[g], nx->stream[g]);
    S.enqueued.assign((size_t)nx->n, 0);
    (void)hipGetLastError();
    vodhip::set_last_error(keep.c_str());
}

}  // namespace

extern "C" {

int vodhip_node_index_search_async(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, int k, int location,
                                   float* out_scores, int64_t* out_ids, void* stream_) {
    if (!nx) return nfail("index is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_check_args(nx, queries, q_dtype, nq, k, location, out_scores, out_ids)) return -1;
    if (nx->n_pending >= 2) return nfail("2 searches are already in flight on this node index: call vodhip_node_index_search_finish first");
    NodeSlot& S = nx->slot[nx->next_slot];
    S.nq = 0;
    S.enqueued.assign((size_t)nx->n, 0);
    if (nq > 0) {
        if (node_enqueue_locked(nx, S, queries, q_dtype, nq, k, location, out_scores, out_ids, stream_)) {
            node_drain_failed(nx, S);
            return -1;
        }
    }
    S.pending = true;
    nx->next_slot ^= 1;
    ++nx->n_pending;
    return 0;
}

int vodhip_node_index_search_finish(vodhip_node_index_t* nx) {
    if (!nx) return nfail("index is NULL");
    // The wait for the devices happens OUTSIDE the mutex: another thread may enqueue the next search into the other slot meanwhile (the
    // batcher's scheduler beside its completion thread).  The slot stays counted as pending until this call is over, so it is not reused.
    std::unique_lock<std::mutex> lk(nx->mu);
    if (nx->n_pending == 0) return nfail("no search is pending on this node index");
    if (nx->finishing) return nfail("another vodhip_node_index_search_finish is running on this node index");
    const int si = (nx->next_slot - nx->n_pending) & 1;
    NodeSlot& S = nx->slot[si];
    nx->finishing = true;
    lk.unlock();
    int rc = 0;
    if (S.nq > 0) {
        rc = node_finish_locked(nx, S);
        if (rc) node_drain_failed(nx, S);  // (the shards whose finish this call did not reach still hold the search)
    }
    lk.lock();
    S.pending = false;
    --nx->n_pending;
    nx->last_finished = si;
    nx->finishing = false;
    return rc;
}

int vodhip_node_index_search(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, int k, int location,
                             float* out_scores, int64_t* out_ids, void* stream_) {
    if (!nx) return nfail("index is NULL");
    {
        std::lock_guard<std::mutex> guard(nx->mu);
        if (nx->n_pending) return nfail("%d asynchronous searches are pending on this node index: finish them first", nx->n_pending);
    }
    if (vodhip_node_index_search_async(nx, queries, q_dtype, nq, k, location, out_scores, out_ids, stream_)) return -1;
    return vodhip_node_index_search_finish(nx);
}

// Listed rows behind the one handle (include/vodhip.h, H2i).  The batch (queries, ids, labels) is brought to host memory once and
// replicated from there; shard g scores the WHOLE list with id_base = g * R - rows of the other shards are out of its range and score
// -inf - and its aligned buffer returns through host memory to devices[0], where the buffers are combined by ownership and, for the
// top-k form, selected once.  Host-synchronous on purpose: a listed request is small, and the route works with or without peer access.
static int node_listed(vodhip_node_index* nx, const void* queries, int q_dtype, int64_t nq, const int64_t* ids, int64_t m, int k,
                       const int32_t* q_labels, int n_per_query, int location, float* out_scores, int64_t* out_ids, void* stream_) {
    if (!nx) return nfail("index is NULL");
    if (m < 1) return nfail("m=%lld: a list holds at least one slot", (long long)m);
    if (k >= 0 && m > VODHIP_MAX_LISTED) return nfail("m=%lld exceeds VODHIP_MAX_LISTED=%d for the top-k form", (long long)m, VODHIP_MAX_LISTED);
    if (k >= 0 && (k < 1 || k > VODHIP_MAX_K)) return nfail("k=%d out of range [1, %d]", k, VODHIP_MAX_K);
    if (nq < 0 || (nq > 0 && (!queries || !ids || !out_scores || (k >= 0 && !out_ids)))) return nfail("invalid query / id / output pointers");
    if (q_dtype < 0 || q_dtype > 2) return nfail("invalid q_dtype %d", q_dtype);
    if (location != VODHIP_HOST && location != VODHIP_DEVICE) return nfail("invalid location %d", location);
    if (q_labels && (n_per_query < 1 || n_per_query > 64)) return nfail("n_per_query must be in [1, 64]");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const int G = nx->n, dev0 = nx->device[0];
    hipStream_t user = location == VODHIP_DEVICE ? (hipStream_t)stream_ : nx->merge_stream;
    const size_t q_bytes = query_bytes(nx, nq, q_dtype), n = (size_t)nq * (size_t)m, lab_bytes = label_bytes(q_labels, nq, n_per_query);
    // 1. the batch in host memory
    std::vector<char> hq, hl;
    std::vector<int64_t> hi;
    const void* q_host = queries;
    const int64_t* ids_host = ids;
    const int32_t* lab_host = q_labels;
    NODE_HIP_OK(hipSetDevice(dev0));
    if (location == VODHIP_DEVICE) {
        hq.resize(q_bytes);
        hi.resize(n);
        hl.resize(lab_bytes);
        NODE_HIP_OK(hipMemcpyAsync(hq.data(), queries, q_bytes, hipMemcpyDeviceToHost, user));
        NODE_HIP_OK(hipMemcpyAsync(hi.data(), ids, n * sizeof(int64_t), hipMemcpyDeviceToHost, user));
        if (q_labels) NODE_HIP_OK(hipMemcpyAsync(hl.data(), q_labels, lab_bytes, hipMemcpyDeviceToHost, user));
        NODE_HIP_OK(hipStreamSynchronize(user));
        q_host = hq.data();
        ids_host = hi.data();
        lab_host = q_labels ? (const int32_t*)hl.data() : nullptr;
    }
    // 2. every shard scores the whole list (the devices run side by side: nothing is waited for until every shard is enqueued)
    std::vector<float> parts((size_t)G * n);
    ShardFanout f(nx);
    const int iq = f.input(q_host, q_bytes), ii = f.input(ids_host, n * sizeof(int64_t)), il = f.input(lab_host, lab_bytes);
    const int io = f.output(parts.data(), n * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            return vodhip_index_score_ids(nx->shard[g], p[iq], q_dtype, nq, (const int64_t*)p[ii], m, g * nx->rows_per_shard, (const int32_t*)p[il], n_per_query,
                                          (float*)p[io], st);
        }))
        return -1;
    // 3. on devices[0]: combine by ownership, select once
    float *d_parts = nullptr, *d_aligned = nullptr, *d_s = nullptr;
    int64_t *d_ids = nullptr, *d_i = nullptr;
    const size_t res = k >= 0 ? (size_t)nq * (size_t)k : 0;
    auto steps = [&]() -> int {
        NODE_HIP_OK(hipMallocAsync((void**)&d_parts, (size_t)G * n * sizeof(float), user));
        NODE_HIP_OK(hipMemcpyAsync(d_parts, parts.data(), (size_t)G * n * sizeof(float), hipMemcpyHostToDevice, user));
        const int64_t* ids0 = ids;
        if (location == VODHIP_HOST) {
            NODE_HIP_OK(hipMallocAsync((void**)&d_ids, n * sizeof(int64_t), user));
            NODE_HIP_OK(hipMemcpyAsync(d_ids, ids_host, n * sizeof(int64_t), hipMemcpyHostToDevice, user));
            ids0 = d_ids;
        }
        float* aligned = out_scores;
        if (k >= 0 || location == VODHIP_HOST) {
            NODE_HIP_OK(hipMallocAsync((void**)&d_aligned, n * sizeof(float), user));
            aligned = d_aligned;
        }
        NODE_HIP_OK(vodhip::launch_combine_listed(d_parts, ids0, (int64_t)n, G, nx->rows_per_shard, aligned, user));
        if (k < 0) {
            if (location == VODHIP_HOST) NODE_HIP_OK(hipMemcpyAsync(out_scores, aligned, n * sizeof(float), hipMemcpyDeviceToHost, user));
        } else {
            float* fs = out_scores;
            int64_t* fi = out_ids;
            if (location == VODHIP_HOST) {
                NODE_HIP_OK(hipMallocAsync((void**)&d_s, res * sizeof(float), user));
                NODE_HIP_OK(hipMallocAsync((void**)&d_i, res * sizeof(int64_t), user));
                fs = d_s;
                fi = d_i;
            }
            NODE_HIP_OK(vodhip::launch_select_listed(aligned, ids0, nq, m, k, 0, fs, fi, user));
            if (location == VODHIP_HOST) {
                NODE_HIP_OK(hipMemcpyAsync(out_scores, fs, res * sizeof(float), hipMemcpyDeviceToHost, user));
                NODE_HIP_OK(hipMemcpyAsync(out_ids, fi, res * sizeof(int64_t), hipMemcpyDeviceToHost, user));
            }
        }
        return 0;
    };
    const int rc = steps();
    const std::string keep = rc ? vodhip_last_error() : "";
    for (void* p : {(void*)d_parts, (void*)d_aligned, (void*)d_s, (void*)d_ids, (void*)d_i})
        if (p) (void)hipFreeAsync(p, user);
    const hipError_t se = hipStreamSynchronize(user);  // (`parts` and the host copies of this frame were sources of copies on `user`)
    if (rc) return nfail("%s", keep.c_str());
    NODE_HIP_OK(se);
    return 0;
}

int vodhip_node_index_score_ids(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, const int64_t* ids, int64_t m,
                                const int32_t* q_labels, int n_per_query, int location, float* out_scores, void* stream) {
    return node_listed(nx, queries, q_dtype, nq, ids, m, -1, q_labels, n_per_query, location, out_scores, nullptr, stream);
}

int vodhip_node_index_search_ids(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, const int64_t* ids, int64_t m,
                                 int k, const int32_t* q_labels, int n_per_query, int location, float* out_scores, int64_t* out_ids,
                                 void* stream) {
    if (k < 0) return nfail("k=%d out of range [1, %d]", k, VODHIP_MAX_K);
    return node_listed(nx, queries, q_dtype, nq, ids, m, k, q_labels, n_per_query, location, out_scores, out_ids, stream);
}

// The weighted sum of listed rows behind the one handle (include/vodhip.h, H2w).  The route of node_listed: the batch through host
// memory to every shard, shard g sums the rows it owns (id_base = g * R), the [nq, dim] sums return through host memory to devices[0]
// and are added there in increasing shard order by the kernel that adds a list's chunks.
int vodhip_node_index_sum_ids(vodhip_node_index_t* nx, const int64_t* ids, const float* weights, int64_t nq, int64_t m, const int32_t* q_labels,
                              int n_per_query, int location, float* out, void* stream_) {
    if (!nx) return nfail("index is NULL");
    if (nx->dtype & VODHIP_L2) return nfail("listed ids are not supported on an L2 index (VODHIP_L2): sum_ids needs an inner-product store");
    if (m < 1) return nfail("m=%lld: a list holds at least one slot", (long long)m);
    if (nq < 0 || (nq > 0 && (!ids || !weights || !out))) return nfail("invalid id / weight / output pointers");
    if (location != VODHIP_HOST && location != VODHIP_DEVICE) return nfail("invalid location %d", location);
    if (q_labels && (n_per_query < 1 || n_per_query > 64)) return nfail("n_per_query must be in [1, 64]");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const int G = nx->n, dev0 = nx->device[0];
    hipStream_t user = location == VODHIP_DEVICE ? (hipStream_t)stream_ : nx->merge_stream;
    const size_t n = (size_t)nq * (size_t)m, n_out = (size_t)nq * (size_t)nx->dim;
    const size_t lab_bytes = label_bytes(q_labels, nq, n_per_query);
    // 1. the batch in host memory
    std::vector<int64_t> hi;
    std::vector<float> hw;
    std::vector<char> hl;
    const int64_t* ids_host = ids;
    const float* w_host = weights;
    const int32_t* lab_host = q_labels;
    NODE_HIP_OK(hipSetDevice(dev0));
    if (location == VODHIP_DEVICE) {
        hi.resize(n);
        hw.resize(n);
        hl.resize(lab_bytes);
        NODE_HIP_OK(hipMemcpyAsync(hi.data(), ids, n * sizeof(int64_t), hipMemcpyDeviceToHost, user));
        NODE_HIP_OK(hipMemcpyAsync(hw.data(), weights, n * sizeof(float), hipMemcpyDeviceToHost, user));
        if (q_labels) NODE_HIP_OK(hipMemcpyAsync(hl.data(), q_labels, lab_bytes, hipMemcpyDeviceToHost, user));
        NODE_HIP_OK(hipStreamSynchronize(user));
        ids_host = hi.data();
        w_host = hw.data();
        lab_host = q_labels ? (const int32_t*)hl.data() : nullptr;
    }
    // 2. every shard sums its own rows (the devices run side by side: nothing is waited for until every shard is enqueued)
    std::vector<float> parts((size_t)G * n_out);
    ShardFanout f(nx);
    const int ii = f.input(ids_host, n * sizeof(int64_t)), iw = f.input(w_host, n * sizeof(float)), il = f.input(lab_host, lab_bytes);
    const int io = f.output(parts.data(), n_out * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            return vodhip_index_sum_ids(nx->shard[g], (const int64_t*)p[ii], (const float*)p[iw], nq, m, g * nx->rows_per_shard, (const int32_t*)p[il],
                                        n_per_query, (float*)p[io], st);
        }))
        return -1;
    // 3. on devices[0]: the shards' sums added in increasing shard order
    float *d_parts = nullptr, *d_out = nullptr;
    auto steps = [&]() -> int {
        NODE_HIP_OK(hipMallocAsync((void**)&d_parts, (size_t)G * n_out * sizeof(float), user));
        NODE_HIP_OK(hipMemcpyAsync(d_parts, parts.data(), (size_t)G * n_out * sizeof(float), hipMemcpyHostToDevice, user));
        float* sum = out;
        if (location == VODHIP_HOST) {
            NODE_HIP_OK(hipMallocAsync((void**)&d_out, n_out * sizeof(float), user));
            sum = d_out;
        }
        NODE_HIP_OK(vodhip::launch_fold_listed_sum(d_parts, G, (int64_t)n_out, nx->dim, nq, (int)nx->dim, sum, user));
        if (location == VODHIP_HOST) NODE_HIP_OK(hipMemcpyAsync(out, sum, n_out * sizeof(float), hipMemcpyDeviceToHost, user));
        return 0;
    };
    const int rc = steps();
    const std::string keep = rc ? vodhip_last_error() : "";
    for (void* p : {(void*)d_parts, (void*)d_out})
        if (p) (void)hipFreeAsync(p, user);
    const hipError_t se = hipStreamSynchronize(user);  // (`parts` was the source of a copy on `user`)
    if (rc) return nfail("%s", keep.c_str());
    NODE_HIP_OK(se);
    return 0;
}

// The log-partition scan behind the one handle (include/vodhip.h, H2p): one ShardFanout of the flat call, the 2 * nq floats per shard
// folded on the host in increasing shard order (partition_fold.h).  No peer copies, no streams beyond the shards' own.
int vodhip_node_index_log_partition(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels,
                                    int n_per_query, float* out_max, float* out_log_rel) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::log_partition_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, out_max, out_log_rel))
        return node_partition_args_fail(msg, q_dtype, beta);
    if (node_scan_refusal(nx, "log_partition")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const int G = nx->n;
    std::vector<float> parts((size_t)G * 2 * (size_t)nq);  // shard g: [max | log_rel] at g * 2 nq
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int io = f.output(parts.data(), 2 * (size_t)nq * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            float* out = (float*)p[io];
            return vodhip_index_log_partition(nx->shard[g], p[iq], q_dtype, nq, beta, (const int32_t*)p[il], n_per_query, out, out + nq, st);
        }))
        return -1;
    vodhip::fold_log_partition(parts.data(), parts.data() + nq, G, 2 * nq, nq, beta, out_max, out_log_rel);
    return 0;
}

// The posterior statistics behind the one handle (include/vodhip.h, H2t): the shape of the log-partition call above with 4 * nq floats
// per shard, folded on the host in increasing shard order, in double (stats_fold.h).
int vodhip_node_index_posterior_stats(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels,
                                      int n_per_query, float* out_max, float* out_log_rel, float* out_mean_rel, float* out_var) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::posterior_stats_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, out_max, out_log_rel, out_mean_rel, out_var))
        return node_partition_args_fail(msg, q_dtype, beta);
    if (node_scan_refusal(nx, "posterior_stats")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const int G = nx->n;
    const size_t n = (size_t)nq;
    std::vector<float> parts((size_t)G * 4 * n);  // shard g: [max | log_rel | mean_rel | var] at g * 4 nq
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int io = f.output(parts.data(), 4 * n * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            float* out = (float*)p[io];
            return vodhip_index_posterior_stats(nx->shard[g], p[iq], q_dtype, nq, beta, (const int32_t*)p[il], n_per_query, out, out + n, out + 2 * n, out + 3 * n, st);
        }))
        return -1;
    vodhip::fold_posterior_stats(parts.data(), parts.data() + n, parts.data() + 2 * n, parts.data() + 3 * n, G, 4 * nq, nq, beta, out_max, out_log_rel,
                                 out_mean_rel, out_var);
    return 0;
}

// The posterior divergence behind the one handle (include/vodhip.h, H2d): the shape of the posterior-stats call above with two query
// sets and 8 * nq floats per shard, folded on the host in increasing shard order, in double (divergence_fold.h).
int vodhip_node_index_posterior_divergence(vodhip_node_index_t* nx, const void* queries_a, const void* queries_b, int q_dtype, int64_t nq,
                                           float beta_a, float beta_b, const int32_t* q_labels, int n_per_query, float* out_max_a,
                                           float* out_log_rel_a, float* out_mean_rel_a, float* out_cross_rel_ab, float* out_max_b,
                                           float* out_log_rel_b, float* out_mean_rel_b, float* out_cross_rel_ba) {
    if (!nx) return nfail("index is NULL");
    float* const outs[8] = {out_max_a, out_log_rel_a, out_mean_rel_a, out_cross_rel_ab, out_max_b, out_log_rel_b, out_mean_rel_b, out_cross_rel_ba};
    if (const char* msg = vodhip::posterior_divergence_args_error(queries_a, queries_b, q_dtype, nq, beta_a, beta_b, q_labels, n_per_query, (const void* const*)outs)) {
        if (!strcmp(msg, "invalid q_dtype")) return nfail("invalid q_dtype %d", q_dtype);
        if (!strncmp(msg, "beta_a", 6)) return nfail("beta_a=%g: %s", (double)beta_a, msg);
        if (!strncmp(msg, "beta_b", 6)) return nfail("beta_b=%g: %s", (double)beta_b, msg);
        return nfail("%s", msg);
    }
    if (node_scan_refusal(nx, "posterior_divergence")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const int G = nx->n;
    const size_t n = (size_t)nq;
    std::vector<float> parts((size_t)G * 8 * n);  // shard g: the eight words, [nq] each, at g * 8 nq
    ShardFanout f(nx);
    const int ia = f.input(queries_a, query_bytes(nx, nq, q_dtype)), ib = f.input(queries_b, query_bytes(nx, nq, q_dtype));
    const int il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int io = f.output(parts.data(), 8 * n * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            float* out = (float*)p[io];
            return vodhip_index_posterior_divergence(nx->shard[g], p[ia], p[ib], q_dtype, nq, beta_a, beta_b, (const int32_t*)p[il], n_per_query, out, out + n,
                                                     out + 2 * n, out + 3 * n, out + 4 * n, out + 5 * n, out + 6 * n, out + 7 * n, st);
        }))
        return -1;
    vodhip::fold_posterior_divergence(parts.data(), G, nq, beta_a, beta_b, outs);
    return 0;
}

// The rank calls behind the one handle (include/vodhip.h, H2r).  One PASS = one ShardFanout of the same flat call, with id_base = the
// shard's first global row.
//   thresholds == NULL  vodhip_index_scan_score_ids of `ids`     -> score_g / row_g  [G][n]
//   else                vodhip_index_count_above (`ids` = the tie ids, may be NULL)  -> count_g [G][n]
// The caller holds nx->mu.
static int node_rank_pass(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, int64_t m, const int64_t* ids, const float* thresholds,
                          const int32_t* q_labels, int n_per_query, float* score_g, int32_t* row_g, int64_t* count_g) {
    const size_t n = (size_t)nq * (size_t)m;
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), ii = f.input(ids, n * sizeof(int64_t));
    const int il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query)), it = f.input(thresholds, n * sizeof(float));
    const int is = f.output(score_g, n * sizeof(float)), ir = f.output(row_g, n * sizeof(int32_t)), ic = f.output(count_g, n * sizeof(int64_t));
    return f.run([&](int g, void* const* p, hipStream_t st) {
        const int64_t base = (int64_t)g * nx->rows_per_shard;
        if (!thresholds)
            return vodhip_index_scan_score_ids(nx->shard[g], p[iq], q_dtype, nq, (const int64_t*)p[ii], m, base, (const int32_t*)p[il], n_per_query,
                                               (float*)p[is], (int32_t*)p[ir], st);
        return vodhip_index_count_above(nx->shard[g], p[iq], q_dtype, nq, (const float*)p[it], (const int64_t*)p[ii], m, base, (const int32_t*)p[il],
                                        n_per_query, (int64_t*)p[ic], st);
    });
}

static int node_rank_check(vodhip_node_index_t* nx, const char* what, const void* queries, int q_dtype, int64_t nq, int64_t m, const void* q_labels,
                           int n_per_query) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::rank_args_error(queries, q_dtype, nq, m, q_labels, n_per_query)) {
        if (!strcmp(msg, "invalid q_dtype")) return nfail("invalid q_dtype %d", q_dtype);
        if (msg[0] == 'm') return nfail("m=%lld: %s", (long long)m, msg + 2);
        return nfail("%s", msg);
    }
    return node_scan_refusal(nx, what);
}

int vodhip_node_index_count_above(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, const float* thresholds, const int64_t* tie_ids,
                                  int64_t m, const int32_t* q_labels, int n_per_query, int64_t* out_counts) {
    if (node_rank_check(nx, "count_above", queries, q_dtype, nq, m, q_labels, n_per_query)) return -1;
    if (nq > 0 && !thresholds) return nfail("thresholds is NULL");
    if (nq > 0 && !out_counts) return nfail("out_counts is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const size_t n = (size_t)nq * (size_t)m;
    std::vector<int64_t> count_g((size_t)nx->n * n);
    if (node_rank_pass(nx, queries, q_dtype, nq, m, tie_ids, thresholds, q_labels, n_per_query, nullptr, nullptr, count_g.data())) return -1;
    vodhip::sum_counts(count_g.data(), (int64_t)n, nx->n, out_counts);
    return 0;
}

int vodhip_node_index_rank_ids(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, const int64_t* ids, int64_t m,
                               const int32_t* q_labels, int n_per_query, int64_t* out_ranks, float* out_scores) {
    if (node_rank_check(nx, "rank_ids", queries, q_dtype, nq, m, q_labels, n_per_query)) return -1;
    if (nq > 0 && !ids) return nfail("ids is NULL");
    if (nq > 0 && !out_ranks) return nfail("out_ranks is NULL");
    if (nq > 0 && !out_scores) return nfail("out_scores is NULL");
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const int G = nx->n;
    const size_t n = (size_t)nq * (size_t)m;
    std::vector<float> score_g((size_t)G * n), thr(n);
    std::vector<int32_t> row_g((size_t)G * n);
    std::vector<uint8_t> present(n);
    std::vector<int64_t> count_g((size_t)G * n);
    if (node_rank_pass(nx, queries, q_dtype, nq, m, ids, nullptr, q_labels, n_per_query, score_g.data(), row_g.data(), nullptr)) return -1;
    vodhip::combine_scan_scores(score_g.data(), row_g.data(), ids, (int64_t)n, G, nx->rows_per_shard, out_scores, present.data());
    vodhip::rank_thresholds(out_scores, present.data(), (int64_t)n, thr.data());
    if (node_rank_pass(nx, queries, q_dtype, nq, m, ids, thr.data(), q_labels, n_per_query, nullptr, nullptr, count_g.data())) return -1;
    vodhip::sum_counts(count_g.data(), (int64_t)n, G, out_ranks);
    return 0;
}

// range_search behind the one handle (H2g).  Pass 1: every shard's sizing call (id_base = its first global row; the flat call maps the
// GLOBAL tie ids to its local rows) -> its own lims; the host adds the list lengths.  Pass 2, with outputs: every shard's full call into
// a block of the longest shard list, then the host concatenates a query's lists in shard order (range_fold.h) - ascending ids.
static int node_range_pass(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, const float* thresholds, const int64_t* tie_ids,
                           const int32_t* q_labels, int n_per_query, int64_t* lims_g, float* scores_g, int64_t* ids_g, int64_t stride) {
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), it = f.input(thresholds, (size_t)nq * sizeof(float));
    const int ii = f.input(tie_ids, (size_t)nq * sizeof(int64_t)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int im = f.output(lims_g, (size_t)(nq + 1) * sizeof(int64_t));
    const int is = f.output(scores_g, (size_t)stride * sizeof(float)), io = f.output(ids_g, (size_t)stride * sizeof(int64_t));
    return f.run([&](int g, void* const* p, hipStream_t st) {
        return vodhip_index_range_search(nx->shard[g], p[iq], q_dtype, nq, (const float*)p[it], (const int64_t*)p[ii], (int64_t)g * nx->rows_per_shard,
                                         (const int32_t*)p[il], n_per_query, (int64_t*)p[im], (float*)p[is], (int64_t*)p[io], stride, st);
    });
}

int vodhip_node_index_range_search(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, const float* thresholds, const int64_t* tie_ids,
                                   const int32_t* q_labels, int n_per_query, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::range_args_error(queries, q_dtype, nq, thresholds, q_labels, n_per_query, lims, out_scores, out_ids, capacity)) {
        if (!strcmp(msg, "invalid q_dtype")) return nfail("invalid q_dtype %d", q_dtype);
        if (!strncmp(msg, "capacity", 8)) return nfail("capacity=%lld: %s", (long long)capacity, msg);
        return nfail("%s", msg);
    }
    if (node_scan_refusal(nx, "range_search")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    lims[0] = 0;
    if (nq == 0) return 0;
    const int G = nx->n;
    std::vector<int64_t> lims_g((size_t)G * (size_t)(nq + 1));
    if (node_range_pass(nx, queries, q_dtype, nq, thresholds, tie_ids, q_labels, n_per_query, lims_g.data(), nullptr, nullptr, 0)) return -1;
    const int64_t total = vodhip::fold_range_lims(lims_g.data(), G, nq, lims);
    if (!out_scores) return 0;
    int64_t stride = 0;  // the longest shard list
    for (int g = 0; g < G; ++g) stride = std::max(stride, lims_g[(size_t)g * (size_t)(nq + 1) + (size_t)nq]);
    if (stride > 0 && capacity > 0) {
        std::vector<float> scores_g((size_t)G * (size_t)stride);
        std::vector<int64_t> ids_g((size_t)G * (size_t)stride);
        if (node_range_pass(nx, queries, q_dtype, nq, thresholds, tie_ids, q_labels, n_per_query, lims_g.data(), scores_g.data(), ids_g.data(), stride)) return -1;
        vodhip::fold_range_lists(lims_g.data(), scores_g.data(), ids_g.data(), stride, G, nq, lims, out_scores, out_ids, capacity);
    }
    if (total > capacity)
        return nfail("range_search: the result holds %lld rows, the outputs %lld (capacity); lims is complete, rows at positions below the capacity are written",
                     (long long)total, (long long)capacity);
    return 0;
}

// The posterior mean behind the one handle (H2m): as above, with nq * dim more floats per shard and fold_posterior_mean behind the fold.
int vodhip_node_index_posterior_mean(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels,
                                     int n_per_query, float* out_max, float* out_log_rel, float* out_mean) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::log_partition_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, out_max, out_log_rel))
        return node_partition_args_fail(msg, q_dtype, beta);
    if (nq > 0 && !out_mean) return nfail("invalid query / output pointers");
    if (node_scan_refusal(nx, "log_partition")) return -1;  // (the name these two refusals have always carried here, as in the flat call)
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const int G = nx->n;
    const size_t dim = (size_t)nx->dim;
    const size_t per_shard = (size_t)nq * (2 + dim);  // shard g: [max | log_rel | mean rows] at g * per_shard
    std::vector<float> parts((size_t)G * per_shard);
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int io = f.output(parts.data(), per_shard * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            float* out = (float*)p[io];
            return vodhip_index_posterior_mean(nx->shard[g], p[iq], q_dtype, nq, beta, (const int32_t*)p[il], n_per_query, out, out + nq, out + 2 * nq, st);
        }))
        return -1;
    vodhip::fold_log_partition(parts.data(), parts.data() + nq, G, (int64_t)per_shard, nq, beta, out_max, out_log_rel);
    vodhip::fold_posterior_mean(parts.data(), parts.data() + nq, parts.data() + 2 * nq, G, (int64_t)per_shard, (int64_t)per_shard, nq, (int64_t)dim, beta,
                                out_max, out_log_rel, out_mean);
    return 0;
}

// The posterior read-out behind the one handle (H2e): as the posterior mean, with n_cols value columns in place of the dim row columns.
// A shard that holds no row returns (-inf, -inf, zeros), the weight-0 part of the fold.
int vodhip_node_index_posterior_expectation(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels,
                                            int n_per_query, float* out_max, float* out_log_rel, float* out_values) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::posterior_expectation_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, out_max, out_log_rel, out_values))
        return node_partition_args_fail(msg, q_dtype, beta);
    if (node_scan_refusal(nx, "posterior_expectation")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (!nx->value_cols) return nfail("posterior_expectation: the index has no value table (vodhip_node_index_set_row_values)");
    if (nx->value_rows != nx->ntotal)
        return nfail("posterior_expectation: the value table holds %lld rows, the index %lld: set the table again after adding rows",
                     (long long)nx->value_rows, (long long)nx->ntotal);
    if (nq == 0) return 0;
    const int G = nx->n;
    const size_t n_cols = (size_t)nx->value_cols;
    const size_t per_shard = (size_t)nq * (2 + n_cols);  // shard g: [max | log_rel | value rows] at g * per_shard
    std::vector<float> parts((size_t)G * per_shard);
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int io = f.output(parts.data(), per_shard * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            float* out = (float*)p[io];
            return vodhip_index_posterior_expectation(nx->shard[g], p[iq], q_dtype, nq, beta, (const int32_t*)p[il], n_per_query, out, out + nq, out + 2 * nq, st);
        }))
        return -1;
    vodhip::fold_posterior_expectation(parts.data(), G, nq, (int64_t)n_cols, beta, out_max, out_log_rel, out_values);
    return 0;
}

// The read-out's gradient behind the one handle (H2b): every shard runs the flat call on its own rows with the GLOBAL forward words, so
// the shard results add (readout_grad_fold.h).  A shard that holds no row returns zeros.
int vodhip_node_index_posterior_expectation_backward(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels,
                                                     int n_per_query, const float* max_score, const float* log_rel, const float* values, const float* grad_values,
                                                     float* out_grad_queries) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::posterior_expectation_backward_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, max_score, log_rel, values,
                                                                            grad_values, out_grad_queries))
        return node_partition_args_fail(msg, q_dtype, beta);
    if (node_scan_refusal(nx, "posterior_expectation_backward")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (!nx->value_cols) return nfail("posterior_expectation_backward: the index has no value table (vodhip_node_index_set_row_values)");
    if (nx->value_rows != nx->ntotal)
        return nfail("posterior_expectation_backward: the value table holds %lld rows, the index %lld: set the table again after adding rows",
                     (long long)nx->value_rows, (long long)nx->ntotal);
    if (nq == 0) return 0;
    const int G = nx->n;
    const size_t n_cols = (size_t)nx->value_cols, dim = (size_t)nx->dim;
    const size_t per_shard = (size_t)nq * dim;
    std::vector<float> parts((size_t)G * per_shard);
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int im = f.input(max_score, (size_t)nq * sizeof(float)), ir = f.input(log_rel, (size_t)nq * sizeof(float));
    const int iy = f.input(values, (size_t)nq * n_cols * sizeof(float)), ig = f.input(grad_values, (size_t)nq * n_cols * sizeof(float));
    const int io = f.output(parts.data(), per_shard * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            return vodhip_index_posterior_expectation_backward(nx->shard[g], p[iq], q_dtype, nq, beta, (const int32_t*)p[il], n_per_query, (const float*)p[im],
                                                               (const float*)p[ir], (const float*)p[iy], (const float*)p[ig], (float*)p[io], st);
        }))
        return -1;
    vodhip::fold_posterior_expectation_backward(parts.data(), G, nq, (int64_t)dim, out_grad_queries);
    return 0;
}

// The read-out's adjoint behind the one handle (H2a): every shard runs the flat call on its own rows with the GLOBAL forward words; its
// result is its slab of rows of the global one, so the slabs are concatenated (readout_adjoint_fold.h).  A shard that holds no row is a
// no-op and owns no slab.
int vodhip_node_index_posterior_adjoint(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels, int n_per_query,
                                        const float* max_score, const float* log_rel, const float* weights, int64_t n_cols, float* out) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::posterior_adjoint_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, max_score, log_rel, weights, n_cols, out))
        return node_partition_args_fail(msg, q_dtype, beta);
    if (node_scan_refusal(nx, "posterior_adjoint")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nx->ntotal == 0) return 0;
    if (nq == 0) {
        std::memset(out, 0, (size_t)nx->ntotal * (size_t)n_cols * sizeof(float));
        return 0;
    }
    const int G = nx->n;
    const size_t slab = (size_t)nx->rows_per_shard * (size_t)n_cols;  // shard g: its rows [lo, hi) at g * slab
    std::vector<float> parts((size_t)G * slab);
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int im = f.input(max_score, (size_t)nq * sizeof(float)), ir = f.input(log_rel, (size_t)nq * sizeof(float));
    const int iw = f.input(weights, (size_t)nq * (size_t)n_cols * sizeof(float));
    const int io = f.output(parts.data(), slab * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            return vodhip_index_posterior_adjoint(nx->shard[g], p[iq], q_dtype, nq, beta, (const int32_t*)p[il], n_per_query, (const float*)p[im], (const float*)p[ir],
                                                  (const float*)p[iw], n_cols, 0, (float*)p[io], st);
        }))
        return -1;
    for (int g = 0; g < G; ++g) vodhip::place_posterior_adjoint_slab(parts.data(), (int64_t)slab, g, nx->ntotal, nx->rows_per_shard, n_cols, out);
    return 0;
}

// The key gradient behind the one handle (H2k): every shard computes its own rows from the GLOBAL (max_score, log_rel, values) and the
// global gradients.  The batch-wide scales are functions of those and of the table's column maxima alone: the node takes the largest
// of the shards' cached maxima - the maxima over all the rows - once and hands it to every shard, so each forms the scales of one index
// holding all the rows (key_grad_fold.h).  The slabs are concatenated as the adjoint's are; nothing is folded.
int vodhip_node_index_posterior_key_gradient(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, float beta, const int32_t* q_labels,
                                             int n_per_query, const float* max_score, const float* log_rel, const float* grad_log_z, const float* values,
                                             const float* grad_values, float* out) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::posterior_key_gradient_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, max_score, log_rel, grad_log_z, values,
                                                                    grad_values, out))
        return node_partition_args_fail(msg, q_dtype, beta);
    if (node_scan_refusal(nx, "posterior_key_gradient")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (grad_values) {
        if (!nx->value_cols) return nfail("posterior_key_gradient: grad_values needs a value table (vodhip_node_index_set_row_values)");
        if (nx->value_rows != nx->ntotal)
            return nfail("posterior_key_gradient: the value table holds %lld rows, the index %lld: set the table again after adding rows",
                         (long long)nx->value_rows, (long long)nx->ntotal);
    }
    if (nx->ntotal == 0) return 0;
    const size_t dim = (size_t)nx->dim;
    if (nq == 0) {
        std::memset(out, 0, (size_t)nx->ntotal * dim * sizeof(float));
        return 0;
    }
    const int G = nx->n;
    const size_t n_cols = grad_values ? (size_t)nx->value_cols : 0;
    const int64_t c_pad = grad_values ? vodhip::readout_c_pad((int64_t)n_cols) : 0;
    std::vector<float> vmax((size_t)c_pad);
    if (grad_values) {
        std::vector<float> vparts((size_t)G * (size_t)c_pad);
        for (int g = 0; g < G; ++g)
            if (vodhip::index_value_vmax(nx->shard[g], vparts.data() + (size_t)g * (size_t)c_pad, c_pad, nx->stream[g])) {
                (void)hipSetDevice(nx->device[0]);
                return nfail("shard %d: %s", g, vodhip_last_error());
            }
        (void)hipSetDevice(nx->device[0]);
        vodhip::fold_key_grad_vmax(vparts.data(), G, c_pad, vmax.data());
    }
    const size_t slab = (size_t)nx->rows_per_shard * dim;  // shard g: its rows [lo, hi) at g * slab
    std::vector<float> parts((size_t)G * slab);
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int im = f.input(max_score, (size_t)nq * sizeof(float)), ir = f.input(log_rel, (size_t)nq * sizeof(float));
    const int ia = f.input(grad_log_z, (size_t)nq * sizeof(float));
    const int iy = f.input(grad_values ? values : nullptr, (size_t)nq * n_cols * sizeof(float)), ig = f.input(grad_values, (size_t)nq * n_cols * sizeof(float));
    const int iv = f.input(grad_values ? vmax.data() : nullptr, (size_t)c_pad * sizeof(float));
    const int io = f.output(parts.data(), slab * sizeof(float));
    if (f.run([&](int g, void* const* p, hipStream_t st) {
            return vodhip::index_posterior_key_gradient(nx->shard[g], p[iq], q_dtype, nq, beta, (const int32_t*)p[il], n_per_query, (const float*)p[im],
                                                        (const float*)p[ir], (const float*)p[ia], (const float*)p[iy], (const float*)p[ig], (const float*)p[iv],
                                                        (float*)p[io], st);
        }))
        return -1;
    for (int g = 0; g < G; ++g) vodhip::place_posterior_adjoint_slab(parts.data(), (int64_t)slab, g, nx->ntotal, nx->rows_per_shard, (int64_t)dim, out);
    return 0;
}

// Posterior sampling behind the one handle (H2s): as above; every shard draws with id_base = its first global row, the lists are
// merged on the host (sample_fold.h).
int vodhip_node_index_sample_posterior(vodhip_node_index_t* nx, const void* queries, int q_dtype, int64_t nq, int k, float beta, uint64_t seed,
                                       int64_t query_offset, const int32_t* q_labels, int n_per_query, float* out_max, float* out_log_rel,
                                       int64_t* out_ids, float* out_scores, float* out_log_p, float* out_log_weight, float* out_keys) {
    if (!nx) return nfail("index is NULL");
    if (const char* msg = vodhip::log_partition_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, out_max, out_log_rel))
        return node_partition_args_fail(msg, q_dtype, beta);
    if (const char* msg = vodhip::sample_posterior_args_error(nq, k, query_offset, 0, out_ids, out_scores, out_log_p, out_log_weight, out_keys)) {
        if (msg[0] == 'k') return nfail("k=%d: %s", k, msg);
        return nfail("%s", msg);
    }
    if (node_scan_refusal(nx, "sample_posterior")) return -1;
    std::lock_guard<std::mutex> guard(nx->mu);
    if (node_labels_refusal(nx, q_labels)) return -1;
    if (nq == 0) return 0;
    const int G = nx->n;
    // shard g, floats: [max | log_rel | scores nq k | log_p | log_weight | keys nq (k + 1)] at g * per_f; ids at g * nq k
    const size_t rows = (size_t)nq * (size_t)k;
    const size_t per_f = 2 * (size_t)nq + 3 * rows + (size_t)nq * (size_t)(k + 1);
    std::vector<float> parts((size_t)G * per_f);
    std::vector<int64_t> ids((size_t)G * rows);
    ShardFanout f(nx);
    const int iq = f.input(queries, query_bytes(nx, nq, q_dtype)), il = f.input(q_labels, label_bytes(q_labels, nq, n_per_query));
    const int io = f.output(parts.data(), per_f * sizeof(float)), ii = f.output(ids.data(), rows * sizeof(int64_t));
    if (f.run([&](int g, void* const* p, hipStream_t st) {  // (the flat call waits for its stream: the shards run one after the other)
            float* o = (float*)p[io];
            return vodhip_index_sample_posterior(nx->shard[g], p[iq], q_dtype, nq, k, beta, seed, query_offset, g * nx->rows_per_shard, (const int32_t*)p[il],
                                                 n_per_query, o, o + nq, (int64_t*)p[ii], o + 2 * nq, o + 2 * nq + rows, o + 2 * nq + 2 * rows,
                                                 o + 2 * nq + 3 * rows, st);
        }))
        return -1;
    vodhip::fold_log_partition(parts.data(), parts.data() + nq, G, (int64_t)per_f, nq, beta, out_max, out_log_rel);
    vodhip::fold_sample_posterior(parts.data() + 2 * nq + 3 * rows, ids.data(), parts.data() + 2 * nq, G, (int64_t)per_f, (int64_t)rows, (int64_t)per_f, nq, k, beta,
                                  out_max, out_log_rel, out_ids, out_scores, out_log_p, out_log_weight, out_keys);
    return 0;
}

int vodhip_node_index_get_stat(vodhip_node_index_t* nx, const char* key, int64_t* out) {
    if (!nx || !key || !out) return nfail("NULL argument");
    std::lock_guard<std::mutex> guard(nx->mu);
    *out = 0;
    if (!strcmp(key, "last_merge_ns") || !strcmp(key, "last_copy_ns_max")) {
        NodeSlot& S = nx->slot[nx->last_finished];
        if (!S.timed || nx->n < 2) return 0;  // (param "profile" was off, or one shard: no exchange, no merge)
        float ms = 0.f;
        if (!strcmp(key, "last_merge_ns")) {
            NODE_HIP_OK(hipSetDevice(nx->device[0]));
            NODE_HIP_OK(hipEventSynchronize(S.merge_ev[1]));
            NODE_HIP_OK(hipEventElapsedTime(&ms, S.merge_ev[0], S.merge_ev[1]));
            *out = (int64_t)((double)ms * 1e6);
            return 0;
        }
        for (int g = 0; g < nx->n; ++g) {
            NODE_HIP_OK(hipSetDevice(nx->device[g]));
            NODE_HIP_OK(hipEventSynchronize(S.copy_ev[2 * g + 1]));
            NODE_HIP_OK(hipEventElapsedTime(&ms, S.copy_ev[2 * g], S.copy_ev[2 * g + 1]));
            *out = std::max<int64_t>(*out, (int64_t)((double)ms * 1e6));
        }
        NODE_HIP_OK(hipSetDevice(nx->device[0]));
        return 0;
    }
    if (!strcmp(key, "last_update_written") || !strcmp(key, "last_update_skipped") || !strcmp(key, "last_update_duplicates")) {
        for (int g = 0; g < nx->n; ++g) {  // (every shard took the last update_rows, with no slot if it owns none)
            int64_t v = 0;
            if (vodhip_index_get_stat(nx->shard[g], key, &v)) return -1;
            *out += v;
        }
        if (!strcmp(key, "last_update_skipped")) *out += nx->update_unrouted;
        NODE_HIP_OK(hipSetDevice(nx->device[0]));
        return 0;
    }
    if (!strcmp(key, "last_remove_removed") || !strcmp(key, "last_remove_skipped") || !strcmp(key, "last_remove_duplicates")) {
        for (int g = 0; g < nx->n; ++g) {  // (every shard took the last remove_rows, with no slot if it owns none)
            int64_t v = 0;
            if (vodhip_index_get_stat(nx->shard[g], key, &v)) return -1;
            *out += v;
        }
        if (!strcmp(key, "last_remove_skipped")) *out += nx->remove_unrouted;
        return 0;
    }
    return nfail("unknown stat '%s'", key);
}

}  // extern "C"
