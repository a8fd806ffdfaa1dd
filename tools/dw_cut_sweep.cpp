// Sweeps the weight-gradient launch planner (csrc/gnf_dw_plan.h: dw_slab_room, the policies, dw_cut) on the host, for a build
// with the sanitizers: every cut of the grid of tests/golden/make_dw_plans.py and of a seeded random sweep (1 .. kMaxGroup
// jobs of 1 .. 4096 x 1 .. 4096, up to 2^20 nodes, 1 .. 4096 workgroups) is checked against what the kernels assume of it.
// Host code only - never loaded into Python, nothing here touches a device:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I graph-normalizing-flows_amd/csrc
//         tools/dw_cut_sweep.cpp -o /tmp/dw_cut_sweep && /tmp/dw_cut_sweep        (one line; an argument: the random count)
#include "gnf_dw_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace gnf;

static long g_cuts = 0, g_wide = 0, g_sk = 0, g_on_tiles = 0, g_xcd = 0, g_direct = 0, g_budget = 0;

#define NEED(cond)                                                                                              \
    do {                                                                                                        \
        if (!(cond)) {                                                                                          \
            std::fprintf(stderr, "dw_cut_sweep: %s fails (line %d): n=%lld nj=%d max_units=%d\n", #cond, __LINE__, \
                         (long long)n, nj, pol.max_units);                                                      \
            std::exit(1);                                                                                       \
        }                                                                                                       \
    } while (0)

static void check(int64_t n, const DwSlabRoom& room, const DwPolicy& pol, int nj, const int32_t* M, const int32_t* N,
                  const bool* bias, bool acc) {
    const DwCut c = dw_cut(n, room, pol, nj, M, N, bias, acc);
    ++g_cuts;
    bool seen[kMaxGroup] = {};
    bool all_in_place = true;
    for (int q = 0; q < nj; ++q) {
        NEED(c.order[q] >= 0 && c.order[q] < nj && !seen[c.order[q]]);
        seen[c.order[q]] = true;
        NEED(c.chunks[q] >= 1 && c.chunks[q] <= room.slab_chunks);
        NEED(!c.in_place[q] || (c.chunks[q] == 1 && !acc));
        all_in_place = all_in_place && c.in_place[q];
    }
    NEED(!c.direct || all_in_place);
    if (!c.wide) {
        NEED(c.units == 0 && c.sk_q == 0 && c.xcd_jobs == 0);
        g_budget += pol.max_units > 0 && n > 0;
        NEED(c.g_gx >= 1 && c.g_gy >= 1 && c.g_nz == nj * room.chunks && c.g_groups >= 1 && c.g_groups * c.g_rpg >= c.g_gy);
        NEED((int64_t)c.g_blocks >= (int64_t)c.g_nz * c.g_groups * c.g_gx * c.g_rpg);
        for (int q = 0; q < nj; ++q) NEED(c.order[q] == q && c.chunks[q] == room.chunks && c.kchunk[q] == room.kchunk);
        g_direct += c.direct;
        return;
    }
    ++g_wide;
    NEED(n > 0 && c.units >= 1 && c.units <= pol.max_units && c.direct == all_in_place);
    int64_t base = 0;
    for (int q = 0; q < nj; ++q) {
        const int e = c.order[q];
        const int tiles = dw_job_tiles(M[e], N[e]);
        NEED(c.unit_base[q] == base && c.gx[q] == (N[e] + WGN - 1) / WGN);
        if (q < c.sk_jobs) {
            NEED(c.sk_q > 0 && c.kchunk[q] == c.sk_q * WGK && !c.in_place[q]);
            base += tiles;
        } else {
            NEED(c.kchunk[q] % WGK == 0 && c.kchunk[q] >= WGK && c.kchunk[q] <= c.max_kchunk);
            NEED((int64_t)c.chunks[q] * c.kchunk[q] >= n && (int64_t)(c.chunks[q] - 1) * c.kchunk[q] < n);
            base += (int64_t)tiles * c.chunks[q];
        }
    }
    NEED(c.unit_base[nj] == base && (c.sk_q > 0 || c.units <= base));
    if (c.sk_q > 0) {
        ++g_sk;
        g_on_tiles += c.light_on_tiles;
        const int64_t total = (int64_t)c.sk_tiles * c.sk_steps;
        NEED(c.sk_steps == (n + WGK - 1) / WGK && c.sk_q <= c.sk_steps && c.sk_jobs >= 1 && c.sk_tiles == c.unit_base[c.sk_jobs]);
        NEED(c.sk_light_base == c.sk_tiles && (int64_t)(c.units - 1) * c.sk_q < total && total <= (int64_t)c.units * c.sk_q);
        int64_t t = 0;
        for (int q = 0; q < c.sk_jobs; ++q)
            for (int k = dw_job_tiles(M[c.order[q]], N[c.order[q]]); k > 0; --k, ++t)  // pieces of tile t <= its job's slabs
                NEED(((t + 1) * c.sk_steps - 1) / c.sk_q - (t * c.sk_steps) / c.sk_q + 1 <= c.chunks[q]);
        NEED(!c.light_on_tiles || (pol.tile_wgs > 0 && c.sk_jobs < nj));
        NEED(c.xcd_jobs == 0);
    } else {
        NEED(c.sk_jobs == 0 && c.sk_tiles == 0 && c.light_on_tiles == 0);
        NEED(c.xcd_jobs >= 0 && c.xcd_jobs <= nj && (c.xcd_jobs == 0 || pol.big_tiles_only));
        for (int q = 0; q < c.xcd_jobs; ++q) NEED(c.chunks[q] == 1 && c.unit_base[q] % 8 == 0);
        g_xcd += c.xcd_jobs > 0;
    }
    g_direct += c.direct;
}

// the job list of a half-step (weight_grad_jobs): the K layers of both nets, then Wq, Wk, Wv, Wo of both nets' attention blocks
struct Net {
    int D;
    std::vector<int32_t> dims;
    int heads, kq, v, out;  // heads == 0: no attention block
    bool graph;
};

static void grid() {
    const Net nets[] = {{8, {4, 32, 32, 4}, 0, 0, 0, 0, false},
                        {64, {32, 256, 256, 256, 256, 32}, 0, 0, 0, 0, false},
                        {200, {100, 2048, 2048, 100}, 0, 0, 0, 0, false},
                        {14, {7, 1280, 1280, 7}, 0, 0, 0, 0, false},
                        {64, {112, 256, 256, 256, 256, 32}, 8, 10, 10, 80, false},
                        {200, {164, 2048, 2048, 100}, 1, 64, 64, 64, false},
                        {64, {112, 256, 256, 256, 256, 32}, 8, 10, 10, 80, true}};
    const int64_t nodes[] = {0, 1, 31, 32, 33, 255, 256, 257, 2718, 3072, 3073, 6000, 16385, 78000, 300000};
    const int64_t units[] = {0, 8, 13, 40, 64, 200, 640};
    const size_t lds = 100 * 1024, lds_min = 67584;
    for (const Net& net : nets) {
        const int K = (int)net.dims.size() - 1, H = net.D / 2;
        int lmax = 0;
        for (int j = 1; j < K; ++j) lmax = lmax > net.dims[j] ? lmax : net.dims[j];
        int32_t M[kMaxGroup], N[kMaxGroup];
        bool bias[kMaxGroup];
        int nj = 0;
        for (int q = 0; q < 2; ++q)
            for (int j = 0; j < K; ++j) M[nj] = net.dims[j], N[nj] = net.dims[j + 1], bias[nj++] = true;
        for (int q = 0; q < 2 && net.heads; ++q) {
            const int nq = net.heads * net.kq, nv = net.heads * net.v;
            M[nj] = H, N[nj] = nq, bias[nj++] = false;
            M[nj] = H, N[nj] = nq, bias[nj++] = false;
            M[nj] = H, N[nj] = net.graph ? nv : net.v, bias[nj++] = false;
            M[nj] = nv, N[nj] = net.out, bias[nj++] = false;
        }
        for (int64_t n : nodes) {
            const DwSlabRoom room = dw_slab_room(n, K, net.dims.data(), lmax);
            const int64_t t16 = (n + 15) / 16, tiles = t16 <= 256 ? t16 : (n + 31) / 32;
            for (int64_t u : units)
                for (int grouped = 0; grouped < 2; ++grouped)
                    for (int thin = 0; thin < 2; ++thin)
                        for (int acc = 0; acc < 2; ++acc) {
                            const DwOptions o{grouped, u, thin};
                            check(n, room, dw_policy_streams(o, K, net.dims.data(), tiles, lds, lds_min), nj, M, N, bias, acc);
                            check(n, room, dw_policy_generic(o, lmax, 256, lds_min), nj, M, N, bias, acc);
                            if (grouped || tiles > kMergedMaxTiles || lmax >= 512) continue;
                            for (int k = 0; k < 4; ++k)
                                check(n, room, dw_policy_merged(o, 256, (int)tiles, lds, k & 1, k >> 1), nj, M, N, bias, acc);
                        }
        }
    }
}

static void random_sweep(unsigned seed, long count) {
    std::mt19937_64 rng(seed);
    auto upto = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    for (long it = 0; it < count; ++it) {
        const int nj = (int)upto(1, kMaxGroup);
        int32_t M[kMaxGroup], N[kMaxGroup];
        bool bias[kMaxGroup];
        const bool small = upto(0, 3) == 0, twins = upto(0, 1) == 0;   // thin layers; many jobs of one shape (hidden layers)
        for (int e = 0; e < nj; ++e) {
            M[e] = (int32_t)upto(1, small ? 300 : 4096), N[e] = (int32_t)upto(1, small ? 300 : 4096), bias[e] = upto(0, 1) != 0;
            if (twins && e > 0 && upto(0, 2) != 0) M[e] = M[0], N[e] = N[0];
        }
        const int64_t n = upto(0, 3) == 0 ? upto(0, 4096) : upto(0, (int64_t)1 << 20);
        const RowCut rc = cut_rows(n, upto(1, 64));
        DwSlabRoom room{rc.chunks, rc.kchunk, rc.chunks};
        if (upto(0, 1) && room.slab_chunks < kTileLightChunks) room.slab_chunks = kTileLightChunks;
        DwPolicy pol{(int)upto(1, 4096), 67584, upto(0, 2) ? 1e30 : (double)upto(1, 2000)};
        pol.big_tiles_only = upto(0, 3) == 0;
        pol.tile_wgs = upto(0, 1) ? (int)upto(1, kMergedMaxTiles) : 0;
        check(n, room, pol, nj, M, N, bias, upto(0, 1) != 0);
    }
}

int main(int argc, char** argv) {
    grid();
    const long grid_cuts = g_cuts;
    random_sweep(20240607u, argc > 1 ? std::atol(argv[1]) : 400000);
    std::printf("dw_cut_sweep: %ld cuts of the grid + %ld random ones hold; wide %ld (stream-K %ld, thin jobs on the tile workgroups "
                "%ld, XCD blocks %ld), direct %ld, grouped though the wide kernel was offered %ld\n",
                grid_cuts, g_cuts - grid_cuts, g_wide, g_sk, g_on_tiles, g_xcd, g_direct, g_budget);
    return 0;
}
