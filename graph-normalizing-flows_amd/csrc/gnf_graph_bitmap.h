// What gnf_graph_stats.hip and gnf_graph_orbits.hip share: the 64-bit adjacency bitmap of a batch read as undirected simple
// graphs (one word per (node, 64 graph-local columns); layout and construction are described in gnf_graph_stats.hip), the
// graph-range helpers, the wave sums and the grid cap.  k_stats_bitmap is DEFINED in gnf_graph_stats.hip and only declared
// here: there is no relocatable device code in this library, a launch from another unit goes through the host-side handle
// that unit registers.
#pragma once
#include "gnf_common.h"

namespace gnf {

static constexpr int kStatsGridMax = 1 << 16;  // workgroups of the grid-stride kernels

// caller-owned workspace of gnf_graph_stats (host only): bitmap uint64 [N][W] | graph id of every node int32 [N]
struct StatsWs {
    size_t bitmap, gid, total;
    int64_t W;
};
inline StatsWs stats_ws(int64_t n_nodes, int32_t max_nodes) {
    StatsWs L;
    L.W = ((int64_t)max_nodes + 63) / 64;
    L.bitmap = 0;
    L.gid = (size_t)n_nodes * (size_t)L.W * sizeof(uint64_t);
    L.total = (L.gid + (size_t)n_nodes * sizeof(int32_t) + 7) / 8 * 8;
    return L;
}

// graph of node i: the last g with node_offsets[g] <= i (empty graphs share their offset with the next one), -1 when i lies
// past node_offsets[n_graphs].  n0 / ng: its first row and size, cut to the node buffer and to the bitmap's columns - offsets
// that do not describe the batch give wrong numbers, never an access outside the arrays.
__device__ __forceinline__ int stats_graph_of(const int32_t* __restrict__ off, int64_t n_graphs, int64_t i) {
    int64_t lo = 0, hi = n_graphs + 1;   // first index with off[idx] > i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)off[mid] <= i) lo = mid + 1; else hi = mid;
    }
    const int64_t g = lo - 1;
    return (g >= 0 && g < n_graphs) ? (int)g : -1;
}
__device__ __forceinline__ void stats_graph_range(const int32_t* __restrict__ off, int g, int64_t n_nodes, int max_nodes,
                                                  int64_t& n0, int& ng) {
    n0 = off[g];
    int64_t n1 = off[g + 1];
    if (n0 < 0) n0 = 0;
    if (n1 > n_nodes) n1 = n_nodes;
    int64_t c = n1 - n0;
    if (c > max_nodes) c = max_nodes;
    ng = c > 0 ? (int)c : 0;
}

// one wave per CSR row i sets bit (i, j - n0) and bit (j, i - n0) of the zeroed bitmap for every entry (receiver i, sender j),
// i != j, inside the graph's window, and writes gid[i]; grid stats_grid((n_nodes + 3) / 4), 256 threads
__global__ __launch_bounds__(256) void k_stats_bitmap(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      int64_t n_nodes, int64_t n_edges, const int32_t* __restrict__ off,
                                                      int64_t n_graphs, int max_nodes, int64_t W,
                                                      unsigned long long* __restrict__ bitmap, int32_t* __restrict__ gid);

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}

inline unsigned stats_grid(int64_t items) {
    if (items < 1) items = 1;
    return (unsigned)(items > kStatsGridMax ? kStatsGridMax : items);
}

// what the per-graph entry points on the bitmap (gnf_graph_components, gnf_graph_subgraph_count, gnf_graph_hashes) ask of csr
// and max_nodes_per_graph (host only; `limit` is the entry point's largest bound)
inline int graph_csr_ok(const char* what, const GnfCsr* csr, int32_t cap, int32_t limit) {
    if (!csr) {
        set_error("%s: null csr", what);
        return GNF_EINVAL;
    }
    if (cap < 0 || cap > limit) {
        set_error("%s: max_nodes_per_graph=%d (0 <= max_nodes_per_graph <= %d)", what, cap, limit);
        return GNF_ESHAPE;
    }
    if (csr->n_nodes < 0 || csr->n_edges < 0 || csr->n_graphs < 0 || csr->n_graphs > 0x7fffffff || csr->n_nodes > 0x7fffffff) {
        set_error("%s: n_nodes=%lld n_edges=%lld n_graphs=%lld", what, (long long)csr->n_nodes, (long long)csr->n_edges,
                  (long long)csr->n_graphs);
        return GNF_ESHAPE;
    }
    if (csr->n_nodes > 0 && (!csr->node_offsets || csr->n_graphs < 1)) {
        set_error("%s: csr->node_offsets / csr->n_graphs are required", what);
        return GNF_EINVAL;
    }
    if (csr->n_graphs > 0 && !csr->node_offsets) {
        set_error("%s: csr->node_offsets is null with n_graphs=%lld", what, (long long)csr->n_graphs);
        return GNF_EINVAL;
    }
    if ((csr->n_nodes > 0 && !csr->rowptr) || (csr->n_edges > 0 && !csr->col)) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    if (csr->n_nodes > 0 && cap == 0) {
        set_error("%s: max_nodes_per_graph=0 with %lld nodes", what, (long long)csr->n_nodes);
        return GNF_ESHAPE;
    }
    return GNF_OK;
}

}  // namespace gnf
