// Random graph models as edge lists on the device (include/gnf_random_graphs.h): G(n, p) / planted partition and
// Barabasi-Albert.  Both are another pass 1 in front of the decoder's scan and pass 2 (gnf_decode_edges.hip): they leave the
// per-graph 64-bit adjacency bitmap and the row counts in the workspace of gnf_edge_ws.h, launch_edge_scan turns the counts into
// rowptr / n_edge / total, and gnf_adj_edges_fill expands the bitmap.  Only the rule that sets the bits is new; it is integer
// arithmetic on gnf_syn_draw throughout.
//   k_rg_planted  k_edge_count's grid and row ownership: one workgroup per (graph, 16-row tile), wave w owns rows 4 w .. 4 w + 3,
//                 lane = column; the graph's hash round is done once per workgroup, the lower node's round once per row or
//                 column, the pair's round once per pair.  One ballot per row and word, one writer per word and count.
//   k_rg_ba       one workgroup of GNF_RG_BA_DRAWS lanes per graph; lane j evaluates draw j of node t; the targets table
//                 [(n - m)][m] and one int32 per node (first-occurrence stamps, later the degrees) sit in dynamic LDS.
// Bounds: a graph's rows [n0, n0 + ng) come from stats_graph_range - inside the node buffer and within max_nodes columns, so
// every bitmap word index is < W and every row < n_nodes; m is clamped into [1, max_m], so every table index is
// < max_nodes * max_m; candidates are clamped below t; block labels are only compared.
#include "gnf_distance_dev.h"
#include "gnf_edge_ws.h"
#include "gnf_graph_bitmap.h"

namespace gnf {

static constexpr uint64_t kRgGolden = 0x9E3779B97F4A7C15ull, kRgM1 = 0xBF58476D1CE4E5B9ull, kRgM2 = 0x94D049BB133111EBull;
static constexpr size_t kRgLdsMax = 160 * 1024;
static constexpr int kRgWaves = GNF_RG_BA_DRAWS / 64;

struct RgArgs {
    uint64_t seed, first_graph;
    const uint64_t* seed_dev;
    const uint64_t *thr_in, *thr_out;
    const int32_t *block, *m_dev;
    const int64_t* node_off;   // [B + 1] (ws)
    unsigned long long* bitmap;
    int32_t* rowcnt;
    int64_t n_nodes, W;
    int32_t max_nodes, n_blocks, max_m, self_loops;
};

// gnf_syn_draw(seed, G, index, stream) = (mix64(mix64(gx ^ M1 (index + 1)) ^ M2 (stream + 1))) >> 32 with the graph's round gx
__device__ __forceinline__ uint64_t rg_graph_round(const RgArgs& a, uint64_t seed_xor) {
    const uint64_t seed = (a.seed_dev ? *a.seed_dev : a.seed) ^ seed_xor;
    return gnf_syn_mix64(seed + kRgGolden * (a.first_graph + (uint64_t)blockIdx.x + 1ull));
}
__device__ __forceinline__ uint64_t rg_index_round(uint64_t gx, uint32_t index) {
    return gnf_syn_mix64(gx ^ (kRgM1 * ((uint64_t)index + 1ull)));
}
__device__ __forceinline__ uint32_t rg_stream_round(uint64_t x, uint32_t stream) {
    return (uint32_t)(gnf_syn_mix64(x ^ (kRgM2 * ((uint64_t)stream + 1ull))) >> 32);
}

// block of local node l < ng at row n0 + l < n_nodes
__device__ __forceinline__ int32_t rg_block_of(const RgArgs& a, int64_t n0, int ng, int l) {
    if (a.block) return a.block[n0 + l];
    if ((uint64_t)ng * (uint64_t)a.n_blocks <= 0xffffffffull) return (int32_t)((uint32_t)l * (uint32_t)a.n_blocks / (uint32_t)ng);
    return (int32_t)((int64_t)l * a.n_blocks / ng);
}

__global__ __launch_bounds__(256) void k_rg_planted(RgArgs a) {
    int64_t n0;
    int ng;
    stats_graph_range(a.node_off, blockIdx.x, a.n_nodes, a.max_nodes, n0, ng);
    if (ng == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int words = (ng + 63) / 64;
    const uint64_t gx = rg_graph_round(a, 0ull);
    const uint64_t thr_in = a.thr_in[blockIdx.x], thr_out = a.thr_out ? a.thr_out[blockIdx.x] : thr_in;
    for (int i0 = blockIdx.y * kEdgeTile; i0 < ng; i0 += gridDim.y * kEdgeTile) {   // (uniform over the workgroup)
        const int rows = ng - i0 < kEdgeTile ? ng - i0 : kEdgeTile;
        const int r0 = wave * kEdgeWaveRows;
        if (r0 >= rows) continue;
        uint64_t xi[kEdgeWaveRows];
        int32_t bi[kEdgeWaveRows];
        int il[kEdgeWaveRows], cnt[kEdgeWaveRows];
        for (int q = 0; q < kEdgeWaveRows; ++q) {
            il[q] = r0 + q < rows ? i0 + r0 + q : i0 + rows - 1;   // rows past the tile's end repeat its last row; not stored
            xi[q] = rg_index_round(gx, (uint32_t)il[q]);
            bi[q] = rg_block_of(a, n0, ng, il[q]);
            cnt[q] = 0;
        }
        for (int w = 0; w < words; ++w) {
            const int j = w * 64 + lane;
            const bool col = j < ng;
            const int jl = col ? j : ng - 1;
            const uint64_t xj = rg_index_round(gx, (uint32_t)jl);
            const int32_t bj = rg_block_of(a, n0, ng, jl);
            for (int q = 0; q < kEdgeWaveRows; ++q) {
                const int i = il[q];
                const uint32_t d = i < jl ? rg_stream_round(xi[q], (uint32_t)jl) : rg_stream_round(xj, (uint32_t)i);
                const uint64_t thr = bi[q] == bj ? thr_in : thr_out;
                const bool edge = col && (i == j ? a.self_loops != 0 : (uint64_t)d < thr);
                const unsigned long long word = __ballot(edge);
                if (r0 + q < rows) {
                    if (lane == 0) a.bitmap[(n0 + i) * a.W + w] = word;
                    cnt[q] += __popcll(word);
                }
            }
        }
        if (lane == 0)
            for (int q = 0; q < kEdgeWaveRows; ++q)
                if (r0 + q < rows) a.rowcnt[n0 + i0 + r0 + q] = cnt[q];
    }
}

__global__ __launch_bounds__(GNF_RG_BA_DRAWS) void k_rg_ba(RgArgs a) {
    extern __shared__ int32_t rg_lds[];   // table [max_nodes * max_m] | mark [max_nodes] | wtot [kRgWaves]
    int64_t n0;
    int ng;
    stats_graph_range(a.node_off, blockIdx.x, a.n_nodes, a.max_nodes, n0, ng);
    if (ng == 0) return;
    int32_t* table = rg_lds;
    int32_t* mark = rg_lds + (size_t)a.max_nodes * a.max_m;
    int32_t* wtot = mark + a.max_nodes;   // first occurrences per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int m = a.m_dev[blockIdx.x];
    m = m < 1 ? 1 : (m > a.max_m ? a.max_m : m);
    const bool grows = ng > m;   // (n <= m: no edges)
    for (int v = tid; v < ng; v += GNF_RG_BA_DRAWS) mark[v] = 0;
    if (grows)
        for (int c = tid; c < m; c += GNF_RG_BA_DRAWS) table[c] = c;   // targets(m) = 0 .. m - 1
    __syncthreads();
    const uint64_t gx = rg_graph_round(a, GNF_RG_BA_SEED_XOR);
    const uint32_t two_m = 2u * (uint32_t)m;
    for (int t = m + 1; t < ng; ++t) {   // (uniform over the workgroup)
        const uint32_t R = two_m * (uint32_t)(t - m);
        const uint32_t d = rg_stream_round(rg_index_round(gx, (uint32_t)t), (uint32_t)tid);
        const uint32_t k = (uint32_t)(((uint64_t)d * R) >> 32);   // < R
        const uint32_t tp = k / two_m, c = k - tp * two_m;        // tp < t - m
        int cand = c < (uint32_t)m ? table[tp * m + c] : m + (int)tp;
        cand = cand < 0 ? 0 : (cand > t - 1 ? t - 1 : cand);
        // first occurrence of a value among the draws of t = the largest stamp on it: later t beat earlier ones (no reset),
        // within t the smallest j wins
        const int32_t stamp = (t << 8) | (GNF_RG_BA_DRAWS - 1 - tid);
        atomicMax(&mark[cand], stamp);
        __syncthreads();
        const bool first = mark[cand] == stamp;
        const unsigned long long word = __ballot(first);
        if (lane == 0) wtot[wave] = __popcll(word);
        __syncthreads();
        int rank = __popcll(word & ((1ull << lane) - 1ull)), accepted = 0;
        for (int w = 0; w < kRgWaves; ++w) {
            rank += w < wave ? wtot[w] : 0;
            accepted += wtot[w];
        }
        int32_t* mine = table + (t - m) * m;
        if (first && rank < m) mine[rank] = cand;
        if (accepted < m && tid == 0) {   // the fallback: the smallest-numbered nodes < t not accepted (t > m: enough of them)
            int r = accepted;
            for (int v = 0; v < t && r < m; ++v)
                if ((mark[v] >> 8) != t) mine[r++] = v;
        }
        __syncthreads();   // targets(t) is read by t + 1; wtot and mark are free again
    }
    // mark becomes the degree: m edges of its own for every t >= m, the loop, then one per appearance as a target
    for (int v = tid; v < ng; v += GNF_RG_BA_DRAWS) mark[v] = (grows && v >= m ? m : 0) + (a.self_loops != 0 ? 1 : 0);
    __syncthreads();
    if (grows) {
        const int entries = (ng - m) * m;
        for (int e = tid; e < entries; e += GNF_RG_BA_DRAWS) {
            const int t = m + e / m;
            int u = table[e];
            u = u < 0 ? 0 : (u > t - 1 ? t - 1 : u);
            atomicOr(&a.bitmap[(n0 + t) * a.W + (u >> 6)], 1ull << (u & 63));
            atomicOr(&a.bitmap[(n0 + u) * a.W + (t >> 6)], 1ull << (t & 63));
            atomicAdd(&mark[u], 1);
        }
    }
    if (a.self_loops != 0)
        for (int v = tid; v < ng; v += GNF_RG_BA_DRAWS) atomicOr(&a.bitmap[(n0 + v) * a.W + (v >> 6)], 1ull << (v & 63));
    __syncthreads();
    for (int v = tid; v < ng; v += GNF_RG_BA_DRAWS) a.rowcnt[n0 + v] = mark[v];
}

}  // namespace gnf

using namespace gnf;

extern "C" {

int gnf_random_graph_edges_count(const GnfRandomGraphSpec* spec, const int32_t* n_node, int64_t n_graphs, int64_t n_nodes,
                                 int32_t max_nodes_per_graph, int32_t* rowptr, int32_t* n_edge, int64_t* total, void* ws,
                                 size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_random_graph_edges_count";
    if (!spec) {
        set_error("%s: null spec", what);
        return GNF_EINVAL;
    }
    if (spec->model != GNF_RG_PLANTED && spec->model != GNF_RG_BARABASI_ALBERT) {
        set_error("%s: model=%d", what, (int)spec->model);
        return GNF_EINVAL;
    }
    const bool ba = spec->model == GNF_RG_BARABASI_ALBERT;
    if (int rc = edge_sizes_ok(what, n_graphs, n_nodes, max_nodes_per_graph)) return rc;
    if (n_graphs > 0x7fffffff) {
        set_error("%s: n_graphs=%lld", what, (long long)n_graphs);
        return GNF_ESHAPE;
    }
    if (!ba && !spec->block && spec->n_blocks < 1) {
        set_error("%s: n_blocks=%d without block labels (n_blocks >= 1)", what, (int)spec->n_blocks);
        return GNF_ESHAPE;
    }
    if (ba && (spec->max_m < 1 || spec->max_m > GNF_RG_MAX_M)) {
        set_error("%s: max_m=%d (1 .. %d)", what, (int)spec->max_m, GNF_RG_MAX_M);
        return GNF_ESHAPE;
    }
    if (!rowptr || !total || !ws || (n_graphs > 0 && (!n_node || !n_edge))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    if (!ba && !spec->thr_in) {
        set_error("%s: the planted model needs thr_in", what);
        return GNF_EINVAL;
    }
    if (ba && !spec->m_dev) {
        set_error("%s: the Barabasi-Albert model needs m_dev", what);
        return GNF_EINVAL;
    }
    const int64_t table = ba ? (int64_t)max_nodes_per_graph * spec->max_m : 0;
    const size_t lds = ba ? (size_t)(table + max_nodes_per_graph + kRgWaves) * sizeof(int32_t) : 0;
    if (table > GNF_RG_BA_TABLE_MAX || lds > kRgLdsMax) {
        set_error("%s: max_nodes_per_graph=%d x max_m=%d: the targets table holds at most %d entries and, with one word per "
                  "node and wave, %zu bytes of LDS", what, max_nodes_per_graph, (int)spec->max_m, GNF_RG_BA_TABLE_MAX, kRgLdsMax);
        return GNF_EUNSUPPORTED;
    }
    const EdgeWs L = edge_ws(n_graphs, n_nodes, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    int64_t* node_off = (int64_t*)((char*)ws + L.node_off);
    RgArgs a = {};
    a.seed = spec->seed, a.first_graph = spec->first_graph, a.seed_dev = spec->seed_dev;
    a.thr_in = spec->thr_in, a.thr_out = spec->thr_out, a.block = spec->block, a.m_dev = spec->m_dev;
    a.node_off = node_off;
    a.bitmap = (unsigned long long*)((char*)ws + L.bitmap);
    a.rowcnt = (int32_t*)((char*)ws + L.rowcnt);
    a.n_nodes = n_nodes, a.W = L.W;
    a.max_nodes = max_nodes_per_graph, a.n_blocks = spec->n_blocks, a.max_m = spec->max_m, a.self_loops = spec->self_loops != 0;
    if (int rc = launch_node_offsets(n_node, n_graphs, node_off, nullptr, st)) return rc;
    if (n_graphs > 0 && n_nodes > 0) {
        if (ba) {
            if (lds > 64 * 1024)
                GNF_ONCE_PER_DEVICE(GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rg_ba),
                                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRgLdsMax)));
            GNF_HIP_TRY(hipMemsetAsync(a.bitmap, 0, L.total - L.bitmap, st));   // the bitmap and the row counts behind it
            hipLaunchKernelGGL(k_rg_ba, dim3((unsigned)n_graphs), dim3(GNF_RG_BA_DRAWS), lds, st, a);
            GNF_LAUNCH_CHECK("k_rg_ba");
        } else {
            hipLaunchKernelGGL(k_rg_planted, edge_grid(n_graphs, max_nodes_per_graph), dim3(256), 0, st, a);
            GNF_LAUNCH_CHECK("k_rg_planted");
        }
    }
    return launch_edge_scan(a.rowcnt, n_graphs > 0 ? n_nodes : 0, node_off, n_graphs, rowptr, n_edge, total, st);
}

}  // extern "C"
