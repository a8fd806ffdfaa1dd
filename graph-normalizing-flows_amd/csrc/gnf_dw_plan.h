// gnf_dw_plan.h - the weight-gradient (dW) launch planner of the backward walk as a pure host computation: which kernel, how
// the node axis of every job is cut, in which order the jobs are launched, which slabs the reduce adds.  No HIP types and no
// pointers: it compiles with a plain C++17 compiler (tools/dw_cut_sweep.cpp runs it under the sanitizers), and
// gnf_train.hip - which lays out the pointers around it (plan_weight_grads) - includes it, so the tile constants below are
// the kernels' own.  Every figure decided here is an index into caller memory or fixes the summation order of a gradient:
// tests/test_dw_plan_cpu.py pins them all (gnf_dw_plan_describe) against plans recorded before this file existed.
#ifndef GNF_DW_PLAN_H_
#define GNF_DW_PLAN_H_
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GNF_DW_HD __host__ __device__
#else
#define GNF_DW_HD
#endif

namespace gnf {

// ---- tile constants shared with the kernels ----------------------------------------------------------------------------
static constexpr int TGM = 128, TGN = 64, TGK = 32;   // the generic / grouped GEMM tile
static constexpr int WGM = 128, WGN = 128, WGK = 32;  // the wide dW kernel's tile
static_assert(TGK == WGK, "cut_rows rounds node chunks for both kernels");
// jobs of one grouped launch.  Per net: K <= 8 layers (GNF_MAX_LAYERS: gnf_train.hip asserts the 8) + Wq, Wk, Wv, Wo of an
// attention block
static constexpr int kMaxGroup = 2 * (8 + 4);
// what fits next to the backward kernel's arguments in one launch (4 KB of kernel arguments)
static constexpr int kMergedGroup = 20;  // message-passing nets of up to 8 layers (16 jobs), attention nets of up to 6 (2 x (6 + 4))
static constexpr int kTileLightChunks = 24;  // most pieces a thin job is cut into for the tile workgroups of a merged launch
static constexpr int kMergedMaxTiles = 192;  // backward tiles of a launch that still leaves CUs for the dW GEMMs

struct WideLayout {
    bool along_n, along_m;  // 1 x 8 waves of 32 x 16 along N / 8 x 1 of 16 x 32 along M / (neither) 4 x 2 waves of 32 x 64
};
GNF_DW_HD inline WideLayout wide_layout(int m_left, int n_left) {  // extents of the tile inside the matrix
    WideLayout l;
    l.along_n = m_left <= 32;
    l.along_m = !l.along_n && n_left <= 32;
    return l;
}

// ---- cutting the node axis ---------------------------------------------------------------------------------------------
struct RowCut {
    int64_t kchunk;  // rows per chunk, a multiple of WGK
    int chunks;
};
// n rows in about c chunks: equal chunks of whole k-steps, and no more of them than it then takes (an empty batch: one)
inline RowCut cut_rows(int64_t n, int64_t c) {
    int64_t kc = (n + c - 1) / c;
    kc = (kc + WGK - 1) / WGK * WGK;
    if (kc < WGK) kc = WGK;
    return RowCut{kc, n > 0 ? (int)((n + kc - 1) / kc) : 1};
}

// The slab room of a backward plan (BwdPlan.chunks / kchunk / slab_chunks): how the grouped kernel cuts the node axis, and
// how many slabs per job the workspace holds - the most ANY cut below may ask for.
struct DwSlabRoom {
    int chunks;
    int64_t kchunk;
    int slab_chunks;  // >= chunks: thin jobs of a merged walk are cut finer (dw_cut, light_on_tiles)
};
// dims[0 .. K]: the layer widths of one net, lmax its widest hidden layer
inline DwSlabRoom dw_slab_room(int64_t n, int K, const int32_t* dims, int lmax) {
    // split of the node axis for dW: every weight gradient of the half-step goes out in ONE grouped launch, so a
    // few chunks already fill the chip; fewer chunks = fewer slabs to write and reduce
    // (measured on the config-2 batch: chunks of 64 / 128 / 256 / 512 nodes give 3.11 / 2.94 / 2.94 / 2.99 ms per step)
    int64_t chunks = (n + 255) / 256;
    if (chunks > 64) chunks = 64;
    // ... but no more than it takes to put ~4 workgroups on every CU: wide layers have the tiles already (2048-wide:
    // 3072 tiles per chunk - a second chunk only added 200 MB of slab traffic per half-step)
    int64_t tiles = 0;
    for (int j = 0; j < K; ++j) tiles += (int64_t)((dims[j] + TGM - 1) / TGM) * ((dims[j + 1] + TGN - 1) / TGN);
    tiles *= 2;
    int64_t enough = (1024 + tiles - 1) / (tiles > 0 ? tiles : 1);
    // ... except that nets with wide hidden layers AND thin first / last layers need slab room for the thin layers' tiles:
    // the wide kernel gives every CU one workgroup that takes whole hidden-layer tiles by stride (one chunk each: the slab
    // is the gradient) and cuts the thin layers' tiles along the node axis so that they ride behind in equal pieces.  With
    // ONE chunk planned they could not be cut: on the data driver's nets 64 of the 256 workgroups carried a third
    // full-length tile (time stamps, round 6: 1 216 k cycles against 813 k for the other 192)
    if (lmax >= 512 && enough < 4) enough = 4;
    if (chunks > enough) chunks = enough;
    if (chunks < 1) chunks = 1;
    const RowCut rc = cut_rows(n, chunks);
    DwSlabRoom r{rc.chunks, rc.kchunk, rc.chunks};
    // merged walk (few tiles, nets the fused kernels hold): room for one short unit of the thin jobs per tile workgroup
    if ((n + 15) / 16 <= kMergedMaxTiles && lmax < 512 && r.slab_chunks < kTileLightChunks) r.slab_chunks = kTileLightChunks;
    return r;
}

// ---- policy: how the dW launch is shaped ---------------------------------------------------------------------------------
// max_units == 0: the 128 x 64 grouped kernel over the plan's chunks (many short workgroups that share CUs with whatever
// else runs).  max_units > 0: the wide kernel in at most that many workgroups, each asking for `lds` bytes of LDS - unless
// the cut this allows would take longer than `budget_us`, in which case the grouped kernel runs after all.
struct DwPolicy {
    int max_units;
    size_t lds;
    double budget_us;
    bool big_tiles_only = false;  // only the jobs with the most tiles count as "costliest" (dw_policy_generic)
    int tile_wgs = 0;  // > 0: the launch that carries this plan has that many backward-tile workgroups with time to spare
                       // (merged walk with the MLP-row stash): a stream-K plan hands them the thin jobs (light_on_tiles)
};
// the library options that force a shape (gnf_set_option: dw_grouped, dw_wide_units, dw_thin_on_dw; 0 = automatic), as read
// in ONE place (dw_options, gnf_train.hip)
struct DwOptions {
    int64_t grouped, wide_units, thin_on_dw;
};
// what every policy of the stream-forking route ends with (shape forcing for the parity tests)
inline DwPolicy dw_policy_forced(const DwOptions& o, DwPolicy pol, size_t lds_min) {
    if (o.grouped) return DwPolicy{0, lds_min, 0.0};
    if (o.wide_units > 0) pol.max_units = (int)o.wide_units, pol.budget_us = 1e30;
    return pol;
}
// Stream-forking route around a fused backward launch.  The fused backward kernel of the NEXT half-step runs beside this
// half-step's dW GEMMs (bwd_tiles workgroups of bwd_lds bytes of LDS: one 16-node tile per workgroup, one workgroup per CU
// by its LDS footprint).  While it leaves CUs idle (config-2 batch: 170 tiles on 256 CUs) the dW launch is sized to exactly
// those: long, equal workgroups, no more of them than there are idle CUs on every XCD (workgroups are dealt round-robin to
// the 8 XCDs of 32 CUs), with enough LDS padding that none fits beside a backward workgroup.  The backward kernel (the
// critical path) then runs undisturbed and the weight gradients finish inside its shadow.  One workgroup too many is costly
// - a backward workgroup that finds no CU waits for a whole dW workgroup - hence the strict cap.  Without enough idle CUs to
// finish in the backward kernel's time, the grouped kernel's many short workgroups spread the contention evenly instead.
// lds_min: the wide kernel's own LDS need.
inline DwPolicy dw_policy_streams(const DwOptions& o, int K, const int32_t* dims, int64_t bwd_tiles, size_t bwd_lds, size_t lds_min) {
    DwPolicy pol{0, lds_min, 0.0};
    if (bwd_tiles > 0 && bwd_tiles <= 192 && bwd_lds > 80 * 1024) {
        // workgroups are dealt round-robin to 32 shader engines of 8 CUs: no engine may get more exclusive workgroups
        // (backward + dW) than it has CUs, or a backward workgroup waits for a whole dW workgroup (measured: the
        // backward kernel then takes 150 instead of 84 us every other half-step)
        pol.max_units = 32 * (8 - (int)((bwd_tiles + 31) / 32));
        const size_t excl = (size_t)160 * 1024 - bwd_lds + 1024;
        if (excl > pol.lds) pol.lds = excl;
        // what the backward kernel takes: recompute + dP chain = 2 x 2 nets x 16 rows x sum(d_j d_j+1) MACs per tile at
        // ~60 % of a CU's fp32 matrix rate (measured: 84 us at 5 x 256-wide layers)
        double macs = 0.0;
        for (int j = 0; j < K; ++j) macs += (double)dims[j] * dims[j + 1];
        // the alternative (grouped kernel sharing every CU) stretches the backward kernel by ~1.3 x
        pol.budget_us = 1.4 * (2.0 * 2.0 * 16.0 * macs * 2.0) / (614e9 * 0.6) * 1e6 + 10.0;
    }
    return dw_policy_forced(o, pol, lds_min);
}
// Stream-forking route with no fused backward launch to fit around (attention nets: the edge kernels of the next half-step
// want every CU, and the grouped kernel's short workgroups share with them better - measured 7.8 vs 8.4 ms per step), or
// behind the generic backward (nets too wide for the fused kernels: the data driver's 2048 x 3 MLPs).  There a hidden
// layer's dW is hundreds of full 128 x 128 tiles over the whole node axis - the wide kernel with ONE chunk per tile (the
// slab IS the gradient: no reduce pass) against the grouped kernel's 128 x 64 tiles + slabs + reduce: wide_fc_train 34.2 ->
// 29.8 ms per step (measured with dw_wide_units = 640 .. 4096).  ONE workgroup per CU, each taking its share of the hidden
// layers' 2 x 256 full tiles by stride with the thin first / last layers' tiles cut into pieces that ride behind through
// slabs of their own.  The count hardly matters (measured 128 .. 512 workgroups: 29.56 .. 29.90 ms per wide_fc_train step,
// best at one per CU): the step is bound by the matrix cores under these kernels' efficiencies, and one workgroup per CU
// leaves the other LDS slot of every CU to the main stream's kernels.
inline DwPolicy dw_policy_generic(const DwOptions& o, int lmax, int cus, size_t lds_min) {
    DwPolicy pol{0, lds_min, 0.0};
    if (lmax >= 512) pol.max_units = cus, pol.budget_us = 1e30, pol.big_tiles_only = true;
    return dw_policy_forced(o, pol, lds_min);
}
// Merged route: the plan rides in the NEXT half-step's launch, beside its `tiles` backward-tile workgroups of `lds` bytes on
// a chip of `cus` CUs (the last half-step's plan gets the whole chip); with the MLP-row stash those tile workgroups end
// early enough to take the thin jobs.  (dw_grouped never gets here: merged_walk_ok.)
inline DwPolicy dw_policy_merged(const DwOptions& o, int cus, int tiles, size_t lds, bool stashed, bool last) {
    int room = last ? cus : cus - tiles;   // CUs the backward tiles of the NEXT launch leave
    if (o.wide_units) room = o.wide_units < room ? (int)o.wide_units : room;  // (shape forcing for the parity tests)
    DwPolicy pol{room, lds, 1e30};
    if (stashed && !last && !o.thin_on_dw) pol.tile_wgs = tiles;  // (the launch that carries this plan walks the next half-step)
    return pol;
}

// ---- the cut ---------------------------------------------------------------------------------------------------------------
// Everything about a dW launch that does not depend on where its buffers are.  Arrays by launch position q (job order[q] of
// the caller's list) unless said otherwise.
struct DwCut {
    bool wide;    // the wide kernel (else the grouped one: every job in room.chunks chunks of room.kchunk rows, list order)
    bool direct;  // every job is written in place: no reduce launch
    int units;    // wide: workgroups of the launch
    int order[kMaxGroup];
    int chunks[kMaxGroup];   // slabs of the job = what the reduce adds;  stream-K jobs: the most pieces of any of their tiles
    int kchunk[kMaxGroup];   // rows per chunk (stream-K jobs: per run)
    int gx[kMaxGroup];
    int unit_base[kMaxGroup + 1];  // prefix sums of units (tiles x chunks; stream-K jobs: tiles) per job
    bool in_place[kMaxGroup];      // ONE chunk and nothing to add to: the job's slab is the gradient itself
    int sk_q, sk_steps, sk_tiles, sk_jobs, sk_light_base, xcd_jobs, light_on_tiles;   // WideGemmT's fields of these names
    int64_t max_kchunk;  // wide: the longest run of rows a workgroup reads of one operand (buffer-path bound)
    int64_t maxred;      // the largest job's elements, bias included (sizes the reduce launch)
    int g_gx, g_gy, g_nz, g_groups, g_rpg;  // the grouped kernel's geometry (k_gemm_dw_grouped)
    unsigned g_blocks;
};

// MFMA tiles per k-slice of the busiest wave of a job's busiest tile (what one step of such a workgroup costs; 16 for a
// full 128 x 128 tile), rounded the way the kernel rounds (1 / 2 / 4 MFMA tiles per side)
inline int dw_job_cost(int M, int N) {
    auto side = [](int len) {
        const int t16 = (len + 15) / 16;
        return t16 > 2 ? 4 : t16;
    };
    const int mt = M < WGM ? M : WGM, nt = N < WGN ? N : WGN;
    const WideLayout l = wide_layout(mt, nt);
    const int wext_m = l.along_m ? 16 : 32, wext_n = l.along_n ? 16 : (l.along_m ? 32 : 64);
    return 2 * side(mt < wext_m ? mt : wext_m) * side(nt < wext_n ? nt : wext_n);  // two waves per SIMD
}
inline int dw_job_tiles(int M, int N) { return ((M + WGM - 1) / WGM) * ((N + WGN - 1) / WGN); }

// what the thin jobs (cost below cmax) take when each of their tiles is cut into c_light pieces, summed over all pieces: a
// step of a full tile (32 rows) takes ~2.1 us at one workgroup per CU (measured), + 4 us of prologue and epilogue per unit
inline double dw_thin_us(int nj, const int* cost, const int* tiles, int cmax, int64_t n, int c_light) {
    double us = 0.0;
    for (int e = 0; e < nj; ++e)
        if (cost[e] != cmax) us += tiles[e] * c_light * ((double)cost[e] / 16.0 * (double)n / c_light / 32.0 * 2.1 + 4.0);
    return us;
}

// One way to run the wide kernel: the grid, how often a costliest / a thin job's tiles are cut, and the estimated time.
struct DwCandidate {
    int grid = 0;       // workgroups (whole chunks with thin workgroups of their own: an upper bound, dw_cut has the count)
    int c_heavy = 0, c_light = 1;
    double est_us = 1e30;
    int sk_q = 0, sk_cmax = 0;  // stream-K: steps per run, the most pieces of a tile
    bool on_tiles = false;      // stream-K: the thin jobs go to the carrying launch's tile workgroups
};
// Whole chunks.  The costliest jobs (the hidden-layer matrices) give the launch its grid: the smallest per-workgroup work
// whose cut of THEM fits max_units; candidates n / k.  Cheaper jobs (thin first / last layers, attention projections) are
// cut into about as many units as there are workgroups and ride behind.
inline DwCandidate dw_whole_chunks(int64_t n, const DwSlabRoom& room, const DwPolicy& pol, int nj, const int* cost, const int* tiles,
                                   int cmax, int heavy_tiles, int light_tiles) {
    DwCandidate w;
    for (int k = room.chunks; k >= 1; --k)
        if ((int64_t)k * heavy_tiles <= pol.max_units) { w.c_heavy = k; break; }
    // (generic backward of wide nets: more whole tiles than workgroups is fine - one chunk each, taken by stride)
    if (w.c_heavy == 0 && pol.big_tiles_only && heavy_tiles > 0) w.c_heavy = 1;
    if (w.c_heavy == 0) return w;
    const RowCut hc = cut_rows(n, w.c_heavy);
    w.c_heavy = hc.chunks;
    w.grid = w.c_heavy * heavy_tiles;
    if (w.grid > pol.max_units) w.grid = pol.max_units;
    bool light_own = false;  // room for the cheap units as workgroups of their own?
    if (light_tiles > 0) {
        light_own = w.grid + light_tiles <= pol.max_units;
        w.c_light = light_own ? (pol.max_units - w.grid) / light_tiles : w.grid / light_tiles;
        w.c_light = w.c_light < 1 ? 1 : (w.c_light > room.chunks ? room.chunks : w.c_light);
    }
    // a step of a full tile (32 rows) takes ~2.1 us at one workgroup per CU (measured); + launch, prologue and epilogue
    // of every unit
    const double heavy_us = (double)cmax / 16.0 * (double)hc.kchunk / 32.0 * 2.1 + 6.0;
    const double light_us = dw_thin_us(nj, cost, tiles, cmax, n, w.c_light);
    w.est_us = light_own ? heavy_us : heavy_us + light_us / w.grid;
    if (light_own) w.grid += light_tiles * w.c_light;
    return w;
}
// Stream-K for the costliest jobs: equal runs of k-steps across tile boundaries instead of whole chunks.
// (24 tiles on 64 workgroups is 2.67 workgroups per tile: cut in whole chunks that is 2 per tile = 48 busy workgroups with
// 43 steps each; as one axis of 24 x 85 steps it is 64 workgroups with 32 steps each.)  sk_q == 0: not applicable.
inline DwCandidate dw_stream_k(int64_t n, const DwSlabRoom& room, const DwPolicy& pol, int nj, const int* cost, const int* tiles,
                               int cmax, int heavy_tiles, int light_tiles) {
    DwCandidate s;
    const int sk_steps = (int)((n + WGK - 1) / WGK);
    if (heavy_tiles <= 0 || heavy_tiles > pol.max_units || sk_steps < 8) return s;
    const int64_t total_steps = (int64_t)heavy_tiles * sk_steps;
    s.sk_q = (int)((total_steps + pol.max_units - 1) / pol.max_units);
    if (s.sk_q < 4) s.sk_q = 4;
    s.grid = (int)((total_steps + s.sk_q - 1) / s.sk_q);
    for (int t = 0; t < heavy_tiles; ++t) {  // pieces of tile t = workgroups whose run touches it
        const int c = (int)(((int64_t)(t + 1) * sk_steps - 1) / s.sk_q - ((int64_t)t * sk_steps) / s.sk_q + 1);
        s.sk_cmax = s.sk_cmax > c ? s.sk_cmax : c;
    }
    const double sk_us = (double)cmax / 16.0 * s.sk_q * 2.0 + 2 * 4.0 + 2.0;
    // (the thin jobs go to the tile workgroups of the carrying launch where it has them: cut for their count)
    // (0.6 / 0.8 / 1.0 / 1.2 units per tile workgroup: 1.874 / 1.862 / 1.858 / 1.903 ms per config2_train step)
    s.on_tiles = pol.tile_wgs > 0 && light_tiles > 0;
    int cl = light_tiles > 0 ? (s.on_tiles ? pol.tile_wgs : s.grid) / light_tiles : 1;
    const int cl_max = s.on_tiles ? room.slab_chunks : room.chunks;
    s.c_light = cl < 1 ? 1 : (cl > cl_max ? cl_max : cl);
    const double light_us = dw_thin_us(nj, cost, tiles, cmax, n, s.c_light);
    s.est_us = s.on_tiles ? sk_us : sk_us + light_us / s.grid;
    // (no better than nothing where the runs are longer than a tile, or the slabs were not planned for that many pieces)
    if (s.sk_q > sk_steps || s.sk_cmax > room.chunks) s.sk_q = 0;
    return s;
}

// has_bias[e]: job e also leaves column sums (a bias gradient).  accumulate: the gradients are added to.
// 1 <= nj <= kMaxGroup jobs.
inline DwCut dw_cut(int64_t n, const DwSlabRoom& room, const DwPolicy& pol, int nj, const int32_t* M, const int32_t* N,
                    const bool* has_bias, bool accumulate) {
    DwCut c = {};
    if (nj < 1 || nj > kMaxGroup) return c;
    int maxM = 1, maxN = 1;
    c.maxred = 1;
    for (int e = 0; e < nj; ++e) {
        maxM = maxM > M[e] ? maxM : M[e];
        maxN = maxN > N[e] ? maxN : N[e];
        const int64_t red = (int64_t)M[e] * N[e] + (has_bias[e] ? N[e] : 0);
        c.maxred = c.maxred > red ? c.maxred : red;
    }
    c.max_kchunk = WGK;
    // ---- wide kernel: cut every job along the node axis so that the workgroups carry about equal MFMA work --------------
    int cost[kMaxGroup], tiles[kMaxGroup];
    DwCandidate pick;
    int cmax = 16;
    if (pol.max_units > 0 && n > 0) {
        int tmax = 1;
        for (int e = 0; e < nj; ++e) {
            cost[e] = dw_job_cost(M[e], N[e]);
            tiles[e] = dw_job_tiles(M[e], N[e]);
            tmax = tmax > tiles[e] ? tmax : tiles[e];
            c.order[e] = e;
        }
        // big_tiles_only: a job with under a quarter of the largest job's tiles is not among the costliest.  (Costs are even,
        // so a demoted job ties with demoted jobs of its own cost only: one sort orders them as sorting before and after did.)
        for (int e = 0; e < nj && pol.big_tiles_only; ++e)
            if (4 * tiles[e] < tmax && cost[e] > 1) cost[e] -= 1;
        for (int a = 1; a < nj; ++a) {  // insertion sort, costliest tiles first (stable): they are dispatched first
            const int v = c.order[a];
            int b = a - 1;
            while (b >= 0 && cost[c.order[b]] < cost[v]) c.order[b + 1] = c.order[b], --b;
            c.order[b + 1] = v;
        }
        if (nj > 0) cmax = cost[c.order[0]];
        int heavy_tiles = 0, light_tiles = 0;
        for (int e = 0; e < nj; ++e) (cost[e] == cmax ? heavy_tiles : light_tiles) += tiles[e];
        pick = dw_whole_chunks(n, room, pol, nj, cost, tiles, cmax, heavy_tiles, light_tiles);
        if (pick.c_heavy > 0) {
            const DwCandidate sk = dw_stream_k(n, room, pol, nj, cost, tiles, cmax, heavy_tiles, light_tiles);
            if (sk.sk_q > 0 && sk.est_us < pick.est_us) {
                const int c_heavy = pick.c_heavy;
                pick = sk, pick.c_heavy = c_heavy;
            }
        }
        c.wide = pick.grid != 0 && !(pick.est_us > pol.budget_us);
    }
    if (!c.wide) {  // the grouped kernel: the plan's chunks for every job, in list order; the tile grid covers the largest job
        for (int e = 0; e < nj; ++e) {
            c.order[e] = e, c.chunks[e] = room.chunks, c.kchunk[e] = (int)room.kchunk;
            // one chunk: its "slab" IS the gradient - written in place, no reduce pass
            c.in_place[e] = room.chunks == 1 && !accumulate;
        }
        c.direct = room.chunks == 1 && !accumulate;
        c.g_gx = (maxN + TGN - 1) / TGN, c.g_gy = (maxM + TGM - 1) / TGM, c.g_nz = nj * room.chunks;
        c.g_groups = c.g_nz >= 32 ? 1 : (32 + c.g_nz - 1) / c.g_nz;   // enough bands that every XCD gets several
        if (c.g_groups > c.g_gy) c.g_groups = c.g_gy;
        c.g_rpg = (c.g_gy + c.g_groups - 1) / c.g_groups;
        c.g_groups = (c.g_gy + c.g_rpg - 1) / c.g_rpg;
        c.g_blocks = 8u * (unsigned)((c.g_nz * c.g_groups + 7) / 8) * (unsigned)(c.g_gx * c.g_rpg);
        return c;
    }
    const int sk_q = pick.sk_q;
    int units = 0;
    // a job in ONE chunk with nothing to add to: its slab is the gradient itself - written in place, nothing for the
    // reduce launch to do for it (every job so: no reduce launch)
    c.direct = !accumulate && sk_q == 0;
    for (int q = 0; q < nj; ++q) {
        const int e = c.order[q];
        const bool heavy = cost[e] == cmax;
        c.gx[q] = (N[e] + WGN - 1) / WGN;
        c.unit_base[q] = units;
        if (sk_q > 0 && heavy) {  // stream-K job: unit_base counts its tiles, chunks = slabs to reduce
            c.chunks[q] = pick.sk_cmax, c.kchunk[q] = sk_q * WGK;
            units += tiles[e];
            c.sk_jobs = q + 1;
        } else {
            const RowCut rc = cut_rows(n, heavy ? pick.c_heavy : pick.c_light);
            c.chunks[q] = rc.chunks, c.kchunk[q] = (int)rc.kchunk;
            units += tiles[e] * rc.chunks;
            c.in_place[q] = !accumulate && rc.chunks == 1;
        }
        c.max_kchunk = c.max_kchunk > c.kchunk[q] ? c.max_kchunk : c.kchunk[q];
        c.direct = c.direct && c.in_place[q];
    }
    c.unit_base[nj] = units;
    if (pol.big_tiles_only && sk_q == 0) {  // XCD blocks for the leading whole-tile jobs (see WideGemmT.xcd_jobs)
        int xj = 0;
        while (xj < nj && cost[c.order[xj]] == cmax && c.chunks[xj] == 1 && tiles[c.order[xj]] % 8 == 0 && c.unit_base[xj] % 8 == 0)
            ++xj;
        c.xcd_jobs = (pick.grid % 8 == 0) ? xj : 0;
    }
    if (sk_q > 0) {
        c.sk_q = sk_q, c.sk_steps = (int)((n + WGK - 1) / WGK), c.sk_tiles = c.unit_base[c.sk_jobs];
        c.sk_light_base = c.unit_base[c.sk_jobs];
        c.light_on_tiles = pick.on_tiles ? 1 : 0;
        c.units = pick.grid;
    } else {
        c.units = pick.grid < units ? pick.grid : units;  // workgroups; units past the grid are picked up by stride
    }
    return c;
}

}  // namespace gnf

#endif  // GNF_DW_PLAN_H_
