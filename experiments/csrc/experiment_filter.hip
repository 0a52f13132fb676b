// libvodhip -- the "tile" ids of the experiment FILTER kernels (`make ABLATION=1 EXPERIMENTS=1` builds only): the one place that maps
// them to kernels.  A search on one of them plans as the persistent kernel (tile 8), whose family runs its bootstrap and dense stages;
// its FILTER stages run the kernel below.  Production builds see the stub in vodhip_internal.h instead.
#include "vodhip_internal.h"

namespace vodhip {

hipError_t launch_filter_ring(int store_dtype, bool pipe, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin,
                              int64_t row_end, int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream);
hipError_t launch_filter_wide(int store_dtype, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin, int64_t row_end,
                              int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream);
bool filter_qres_supports(int64_t dim_pad);
hipError_t launch_filter_qres(int store_dtype, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin, int64_t row_end,
                              int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream);
bool filter_ksplit_supports(int64_t dim_pad);
hipError_t launch_filter_ksplit(int store_dtype, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin, int64_t row_end,
                                int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream);

template <int ID>
hipError_t launch_experiment(int store_dtype, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin, int64_t row_end,
                             int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream) {
    if constexpr (ID == 10 || ID == 11)  // the deep LDS ring; 11: fragments read one k-step ahead
        return launch_filter_ring(store_dtype, ID == 11, store, q_pad, dim_pad, row_begin, row_end, nq, nq_pad, ws, stream);
    else if constexpr (ID == 12)  // the 384 x 256 workgroup tile
        return launch_filter_wide(store_dtype, store, q_pad, dim_pad, row_begin, row_end, nq, nq_pad, ws, stream);
    else if constexpr (ID == 13 || ID == 15 || ID == 16)  // 8-phase K loop variants: B0 re-read in phase 4 (13), LDS-DMA lead 6 / 5 (15 / 16)
        return launch_filter_8phase(store_dtype, ID == 15 ? 6 : ID == 16 ? 5 : 7, ID != 13, store, q_pad, dim_pad, row_begin, row_end, nq, nq_pad, ws, stream);
    else {  // the query tile resident in registers (17; dim_pad 384 / 768), with a K-split wave pair (18; dim_pad 768); shapes they do not
            // take run the production 8-phase kernel
        const bool subset = ws.extra.row_label != nullptr;
        if (ID == 17 && !subset && filter_qres_supports(dim_pad))
            return launch_filter_qres(store_dtype, store, q_pad, dim_pad, row_begin, row_end, nq, nq_pad, ws, stream);
        if (ID == 18 && !subset && filter_ksplit_supports(dim_pad))
            return launch_filter_ksplit(store_dtype, store, q_pad, dim_pad, row_begin, row_end, nq, nq_pad, ws, stream);
        return launch_filter_8phase(store_dtype, 7, true, store, q_pad, dim_pad, row_begin, row_end, nq, nq_pad, ws, stream);
    }
}

FilterStageFn experiment_filter(PlanTunables& t) {
    FilterStageFn f = nullptr;
    switch (t.tile) {
        case 10: f = launch_experiment<10>; break;
        case 11: f = launch_experiment<11>; break;
        case 12: f = launch_experiment<12>; break;
        case 13: f = launch_experiment<13>; break;
        case 15: f = launch_experiment<15>; break;
        case 16: f = launch_experiment<16>; break;
        case 17: f = launch_experiment<17>; break;
        case 18: f = launch_experiment<18>; break;
        default: return nullptr;
    }
    if (t.tile <= 12) t.tile_order = 1;  // 10 - 12 address the store without the stage permutation
    t.tile = (int64_t)FilterKernel::Persistent;
    return f;
}

}  // namespace vodhip
