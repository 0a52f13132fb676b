// The planner of a search (search_plan.h): host code only, compiled by the host compiler (see the Makefile).
#include "search_plan.h"

#include <stdint.h>

#include <algorithm>

namespace vodhip {

namespace {

void make_safe_schedule(int64_t n, int64_t cap, std::vector<Stage>& st) {
    const int64_t step = std::max<int64_t>(ROW_ALIGN, cap / ROW_ALIGN * ROW_ALIGN);
    for (int64_t b = 0; b < n; b += step) st.push_back({ST_DENSE, b, std::min(n, b + step), 0, 0, 0});
}

// dense head of <= cap rows, then FILTER stages that grow by 1 + cap / 4k (each emits ~ (growth - 1) k survivors per query for
// exchangeable row order): the schedule for searches that cannot use the bootstrap (subset filters; k too large for cap)
void make_geometric_schedule(int64_t n, int k, int64_t cap, std::vector<Stage>& st) {
    int64_t b = std::min(n, std::max<int64_t>(ROW_ALIGN, std::min<int64_t>(cap, 2048) / ROW_ALIGN * ROW_ALIGN));
    if (b < k && b < n) return make_safe_schedule(n, cap, st);
    st.push_back({ST_DENSE, 0, b, 0, 0, 0});
    const double growth = std::min(8.0, std::max(1.25, 1.0 + (double)cap / (4.0 * k)));
    while (b < n) {
        const int64_t e = std::min(n, round_up(std::max((int64_t)((double)b * growth), b + ROW_ALIGN), ROW_ALIGN));
        st.push_back({ST_FILTER, b, e, 0, 0, 0});
        b = e;
    }
}

// `recovery` > 0: pass number after a candidate-list overflow - no bootstrap (the thresholds are seeded from the previous
// result), 2^(recovery-1) equal FILTER stages, and the exhaustive schedule once a stage would be <= cap rows.
void make_schedule(int64_t n, int k, const PlanTunables& t, const FilterGeometry& g, int64_t nq_pad, bool safe, int recovery, std::vector<Stage>& st) {
    const int64_t cap = t.cand_cap;
    if (n <= 0) return;
    int64_t dense_limit = std::max(t.dense_rows, round_up(k, ROW_ALIGN));
    dense_limit = std::min(dense_limit, cap / ROW_ALIGN * ROW_ALIGN);
    if (safe || n <= dense_limit) return make_safe_schedule(n, cap, st);
    if (recovery > 0) {
        const int64_t n_st = 1ll << std::min(recovery - 1, 30);
        const int64_t rows = round_up((n + n_st - 1) / n_st, ROW_ALIGN);
        if (rows <= cap) return make_safe_schedule(n, cap, st);
        for (int64_t b = 0; b < n; b += rows) st.push_back({ST_FILTER, b, std::min(n, b + rows), 0, 0, 0});
        return;
    }
    const int64_t bm = g.rows, rg = g.group_rows;
    // 4k groups wanted, 2k needed: the k-th largest of G group maxima is exceeded by a fraction -ln(1 - k/G) / rg of the rows,
    // ~1.15 k/S at G = 4k, 1.39 k/S at G = 2k (the stage-size bound below allows 1.6 k/S), and it blows up as G approaches k
    int64_t kp = 64;
    while (kp < k) kp <<= 1;
    // one candidate slot per group, and the select kernel takes the group maxima in ONE round of its largest buffer
    const int64_t g_max = std::min<int64_t>(cap, 8192 - kp);
    const int64_t s_max = std::min(rg * g_max, n / 2) / bm * bm;
    const int64_t s_need = round_up(std::max<int64_t>(2 * rg * (int64_t)k, 2048), bm);
    if (s_max < s_need) {  // no usable bootstrap (few rows, or k too large for cap): all dense when that is a few launches
        if (n <= 64 * cap) return make_safe_schedule(n, cap, st);
        return make_geometric_schedule(n, k, cap, st);
    }
    const int64_t s_min = std::min(s_max, round_up(std::max<int64_t>(4 * rg * (int64_t)k, 2048), bm));
    // Round 6: the survivor path of the FILTER epilogue is 7-10 % of a C3 batch (kernels_mips_8phase.hip), and a stage lets ~ growth * k
    // rows per query pass: on a large store searched with a large batch, more and smaller stages behind a smaller bootstrap pay (10 M x
    // 768, nq 1024: growth 3 + N / 192 = 6 launches against growth 8 + N / 96 = 4: -2.0 %, exact-f32 -2.1 %, clustered rows -1.9 %).  At
    // 512 queries and fewer (half the survivors per corpus tile) and on small stores a stage's own cost - a select launch, a partial round
    // of the persistent grid - weighs as much: measured +-0.4 % (5 M / 40 M x 1024 at nq 512, 10 M at nq 256, 1.25 M), the round-3 rule
    // stays there (profiles/r06_ab_epilogue.txt).
    const bool many_small_stages = n >= 4000000 && nq_pad > 512;
    const int64_t sdiv = t.sample_div > 0 ? t.sample_div : (many_small_stages ? 192 : 96);
    int64_t s = std::min(s_max, std::max(s_min, round_up(n / std::max<int64_t>(sdiv, 2), bm)));
    int64_t round_rows = ROW_ALIGN;  // corpus rows ONE round of the persistent grid covers (one 256 x 256 tile per CU)
    if (g.persistent) {
        round_rows = std::max<int64_t>(1, std::max(1, t.n_cu) / std::max<int64_t>(1, nq_pad / 256)) * bm;
        // the persistent kernel runs one workgroup per CU: a bootstrap of r.x "rounds" of tiles costs as much as r+1 full ones.
        // Whole rounds only: down when that keeps >= 4k groups (a cheaper bootstrap), up otherwise (a tighter bound for free)
        const int64_t down = s / round_rows * round_rows, up = round_up(s, round_rows);
        if (down >= s_min) s = down;
        else if (up <= s_max) s = up;
    }
    // S sampled rows at stride (n-1)/(S-1): the last one is row (S-1)*rstride <= n-1, all distinct (S <= n/2)
    st.push_back({ST_GMAX, 0, 0, s / bm, (n - 1) / (s - 1), s / rg});
    // however the rows are ordered, rows [b, e) hold about k * (e - b) / S scores above the bootstrap bound (the sample is
    // stratified over the whole store): a stage never covers more rows than the candidate lists can take with 60 % headroom
    const int64_t rows_safe = std::max<int64_t>(ROW_ALIGN, (int64_t)((double)cap * (double)s / (1.6 * (double)k)) / ROW_ALIGN * ROW_ALIGN);
    const size_t n_head = st.size();
    auto plan = [&](double growth) {
        st.resize(n_head);
        int64_t b = 0, calibrated = s;
        while (b < n) {
            int64_t rows = std::min(rows_safe, round_up((int64_t)((double)calibrated * growth), ROW_ALIGN));
            // stages held down by the capacity bound share what is left evenly (40 M x 1024 at growth 3: 3 x 10.06 M + a 0.38 M tail otherwise)
            if (rows == rows_safe && n - b > rows) {
                const int64_t m = (n - b + rows_safe - 1) / rows_safe;
                rows = std::min(rows_safe, round_up((n - b + m - 1) / m, ROW_ALIGN));
            }
            // whole rounds of the persistent grid: a stage of r.x rounds costs r + 1 (its last round runs on a fraction of the CUs), so
            // only the LAST stage of a search may end inside a round (round 4; the capacity bound rows_safe only ever rounds DOWN)
            if (rows > round_rows) rows = rows / round_rows * round_rows;
            int64_t e = std::min(n, b + rows);
            if (n - e < rows / 4 && n - b <= rows_safe) e = n;  // no short tail stage
            st.push_back({ST_FILTER, b, e, 0, 0, 0});
            b = e;
            calibrated = e;
        }
    };
    plan(std::min(256.0, std::max(1.25, t.growth_x100 > 0 ? t.growth_x100 / 100.0 : (many_small_stages ? 3.0 : 8.0))));
    // A store of ~10-20 sample sizes comes out as a short first stage followed by ONE stage with all the rest (the 1.25 M-row shard
    // of the headline: 131 k + 1,119 k rows).  Three stages at growth 4 (65 k + 327 k + 858 k) measure 1.3 % faster there, six out of
    // six interleaved runs (profiles/r03_ab_growth.txt); stores that already get three or more stages are unaffected (10 M rows: growth
    // 4 is 0.5 % slower than 8, so the default stays).
    if (t.growth_x100 <= 0 && st.size() == n_head + 2 && (st[n_head + 1].e - st[n_head + 1].b) > 6 * (st[n_head].e - st[n_head].b)) plan(4.0);
}

}  // namespace

SearchPlan plan_search(int64_t ntotal, int k, int64_t nq, const PlanTunables& t, bool subset, bool safe, int recovery) {
    SearchPlan p;
    // auto: up to 128 queries the search is HBM-bound: 256 corpus rows x 64 / 128 queries per workgroup on a 3-slot LDS
    // ring (few query bytes per corpus byte through the LDS-DMA path); above, the persistent 256x256 tile on
    // v_mfma_f32_16x16x32 (8; variant 9 staggers the two waves of every SIMD by one k-step: measured equal or 1-2 % slower)
    const FilterKernel base = t.tile != 0 ? (FilterKernel)t.tile
                                          : nq > 128 ? FilterKernel::Persistent : (nq > 64 ? FilterKernel::Generic256x128 : FilterKernel::Generic256x64);
    const FilterGeometry& g = geometry(base);
    p.bn = g.cols;
    const int64_t nq_pad = round_up(std::min(MAX_NQ_PER_PASS, nq), p.bn);  // of the first (largest) pass
    std::vector<Stage>& st = p.stages;
    // group maxima would include ineligible rows: a subset search runs the exhaustive-free geometric schedule instead
    // (dense head of <= cap rows, then FILTER stages growing by `growth`)
    if (subset && !safe && recovery == 0) make_geometric_schedule(ntotal, k, t.cand_cap, st);
    else make_schedule(ntotal, k, t, g, nq_pad, safe, recovery, st);
    // ONE q-tile: every corpus line is read by exactly one workgroup, once - fetch it with the `nt` policy so it does not
    // push the query tile out of L2 (measured -2 % at nq = 256 on 10 M rows; +8 % with 4 q-tiles sharing the lines, so only here)
    p.corpus_nt = g.persistent && nq_pad == 256;
    // The order in which the FILTER stages walk the store's 256-row super-tiles: a low-discrepancy permutation (position p ->
    // super-tile p * P mod T, P ~ 0.618 T coprime to T), so that every stage - any run of consecutive positions - is spread evenly
    // over the whole store.  The reference ingests documents in corpus order (build.py:65-73): with contiguous stages a topic that
    // only the LAST stage contains meets a threshold calibrated without it, and all its tiles are scanned at the same moment
    // (bench.py --data clustered: 1.22x the i.i.d. time, L2-miss traffic 1.9x).  Only when every stage after the bootstrap is a FILTER
    // stage (they must tile the store together); results do not depend on the order.
    bool all_filter = !st.empty();
    for (const Stage& sg : st) all_filter = all_filter && (sg.kind == ST_FILTER || sg.kind == ST_GMAX);
    const int64_t T = (ntotal + ROW_ALIGN - 1) / ROW_ALIGN;
    if (all_filter && t.tile_order == 0 && T >= 8) {
        const int64_t P = tile_order_multiplier(T);
        if (P > 1) {
            p.perm_mul = P;
            p.perm_mod = T;
        }
    }
    // The FILTER stages of auto batches above 128 queries run the 8-phase K loop (tile 14: C3 -2.4 %, C4 shard -4.0 %; with ONE query tile
    // and the corpus stream on the `nt` policy C2 -3.5 %, nq 256 on 10 M rows -2.7 %: profiles/r05_ab_8phase.txt, r05_ab_one_query_tile.txt);
    // its subset instantiation spilled through round 6a and is 4-5 % slower than tile 8 on filtered searches since it no longer does
    // (2.5 M x 768, a quarter of the rows eligible: 3.95-3.99 vs 3.78-3.80 ms, experiments/tools/probe_subset_tile.py): they stay on
    // tile 8, as does the bootstrap
    const bool auto_8phase = t.tile == 0 && nq > 128 && !subset;
    // short FILTER stages of auto batches do not fill the CUs with 256x256 tiles: those launches run on 128x128 tiles, 2 workgroups per CU
    if (t.tile == 0 && g.persistent) p.small_tiles = t.small_chunk_tiles;
    for (Stage& sg : st) {
        sg.kernel = base;
        if (sg.kind == ST_DENSE && g.persistent) sg.kernel = FilterKernel::Generic128;  // nq_pad is a multiple of 256, which it divides
        if (sg.kind == ST_GMAX && base == FilterKernel::EightPhase) sg.kernel = FilterKernel::Persistent;  // (FILTER stages only)
        if (sg.kind == ST_FILTER && auto_8phase) sg.kernel = FilterKernel::EightPhase;
        // S sampled rows at offset + i * rstride, i < S: the (ntotal - 1) % rstride-ish rows the integer stride leaves out are split
        // between the head and the tail of the store
        if (sg.kind == ST_GMAX) sg.sample_offset = ((ntotal - 1) - (sg.n_tiles * geometry(sg.kernel).rows - 1) * sg.rstride) / 2;
    }
    // the survivor rings of the 8-phase kernel, sized for its largest stage: a FILTER stage against a threshold calibrated on C rows
    // passes ~k * rows / C rows per query (the k-th best of C rows; 1.15-1.39 x that behind the bootstrap's group maxima); a
    // recovery pass's thresholds come from a result over the whole store
    double per_query = 0.0;
    int64_t calibrated = ntotal;
    for (const Stage& sg : st) {
        if (sg.kind == ST_GMAX) calibrated = sg.n_tiles * geometry(sg.kernel).rows;
        if (sg.kind == ST_FILTER && sg.kernel == FilterKernel::EightPhase)
            per_query = std::max(per_query, 1.4 * k * (double)(sg.e - sg.b) / (double)std::max<int64_t>(1, calibrated));
        if (sg.kind != ST_GMAX) calibrated = sg.e;
    }
    if (per_query > 0.0) p.ring = t.survivor_ring > 0 ? t.survivor_ring : survivor_ring_records(per_query, nq_pad, t.n_cu);
    return p;
}

int64_t survivor_ring_records(double per_query, int64_t nq_pad, int n_cu) {
    const int64_t n_qt = std::max<int64_t>(1, nq_pad / 256);
    const int64_t unit = 8 * n_qt;  // the 8-phase launcher's grid: whole multiples of 8 workgroups per query tile
    const int64_t grid = std::max(unit, std::max(1, n_cu) / unit * unit);
    const double per_wave = per_query * 64.0 / (double)(2 * grid / n_qt);
    return std::min<int64_t>(MAX_AUTO_SURVIVOR_RING, round_up((int64_t)(2.0 * per_wave) + 64, 64));
}

// The multiplier of the low-discrepancy stage order over T super-tiles: position p -> super-tile (p * P) mod T with P the largest
// integer <= T / golden ratio that is coprime to T (a bijection of [0, T); consecutive positions land ~0.618 T apart, so any run of L
// positions leaves gaps of O(T / L) - three-distance theorem).  <= 1: no permutation.
int64_t tile_order_multiplier(int64_t T) {
    if (T < 8) return 0;
    // Candidates around T / golden ratio; among those coprime to T the one whose continued fraction P / T has the smallest largest
    // partial quotient: a run of L consecutive multiples of P (mod T) then leaves gaps within a small factor of T / L at EVERY scale L
    // (three-distance theorem; a candidate that merely is coprime can sit next to a fraction with a small denominator and leave gaps
    // 12x the mean - seen at T = 99,684).
    const int64_t P0 = (int64_t)((double)T * 0.6180339887498949);
    int64_t best = 0, best_q = INT64_MAX;
    for (int64_t d = 0; d <= 64; ++d) {
        for (int sgn = 0; sgn < 2; ++sgn) {
            const int64_t P = sgn ? P0 - d : P0 + d;
            if (P <= 1 || P >= T || (d == 0 && sgn)) continue;
            int64_t a = T, b = P, worst = 0;
            bool first = true;
            while (b) {  // Euclid: the partial quotients of T / P
                const int64_t quo = a / b, rem = a % b;
                if (!first) worst = std::max(worst, quo);  // (the first is floor(T / P) = 1 by construction)
                first = false;
                a = b;
                b = rem;
            }
            if (a != 1) continue;  // not coprime
            if (worst < best_q) {
                best_q = worst;
                best = P;
            }
        }
    }
    return best;
}

}  // namespace vodhip
