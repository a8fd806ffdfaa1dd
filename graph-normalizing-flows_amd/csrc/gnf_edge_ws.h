// What the producers of an adjacency bitmap for gnf_adj_edges_fill share (gnf_decode_edges.hip: the decoders' pass 1;
// gnf_random_graphs.hip: the random graph models): the caller-owned workspace layout, the grid and row ownership of the
// (graph, 16-row tile) kernels, the host-side size rules and the launcher of the scan that turns row counts into rowptr /
// n_edge / total.  gnf_adj_edges_workspace_bytes is edge_ws(...).total.
#pragma once
#include "gnf_common.h"

namespace gnf {

static constexpr int kEdgeTile = 16;      // rows per workgroup pass; 4 waves x 4 rows
static constexpr int kEdgeWaveRows = 4;

// caller-owned workspace of the two calls (host only): node_off int64 [B + 1] | bitmap uint64 [N][W] | rowcnt int32 [N]
// (the scan keeps its partial sums in LDS)
struct EdgeWs {
    size_t node_off, bitmap, rowcnt, total;
    int64_t W;
};
inline EdgeWs edge_ws(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes) {
    EdgeWs L;
    L.W = ((int64_t)max_nodes + 63) / 64;
    L.node_off = 0;
    L.bitmap = (size_t)(n_graphs + 1) * sizeof(int64_t);
    L.rowcnt = L.bitmap + (size_t)n_nodes * (size_t)L.W * sizeof(uint64_t);
    L.total = (L.rowcnt + (size_t)n_nodes * sizeof(int32_t) + 7) / 8 * 8;
    return L;
}

inline int edge_sizes_ok(const char* what, int64_t n_graphs, int64_t n_nodes, int32_t max_nodes) {
    if (n_graphs < 0 || n_nodes < 0 || max_nodes < 0) {
        set_error("%s: n_graphs=%lld n_nodes=%lld max_nodes_per_graph=%d", what, (long long)n_graphs, (long long)n_nodes, max_nodes);
        return GNF_ESHAPE;
    }
    if (n_nodes > 0 && n_graphs > 0 && max_nodes == 0) {
        set_error("%s: max_nodes_per_graph=0 with %lld nodes", what, (long long)n_nodes);
        return GNF_ESHAPE;
    }
    if (n_nodes * (int64_t)max_nodes > INT32_MAX) {
        set_error("%s: n_nodes=%lld x max_nodes_per_graph=%d exceeds the int32 edge ids", what, (long long)n_nodes, max_nodes);
        return GNF_ESHAPE;
    }
    return GNF_OK;
}

inline dim3 edge_grid(int64_t n_graphs, int32_t max_nodes) {
    int64_t tiles = ((int64_t)max_nodes + kEdgeTile - 1) / kEdgeTile;
    if (tiles > 65535) tiles = 65535;   // (the kernels stride over a graph's tiles)
    return dim3((unsigned)n_graphs, (unsigned)tiles);
}

// k_edge_scan (gnf_decode_edges.hip), one workgroup: rowptr = exclusive prefix of rowcnt [n_nodes], n_edge [n_graphs] from
// node_off, *total.  n_nodes == 0 writes rowptr[0] = 0 and *total = 0.
int launch_edge_scan(const int32_t* rowcnt, int64_t n_nodes, const int64_t* node_off, int64_t n_graphs, int32_t* rowptr,
                     int32_t* n_edge, int64_t* total, hipStream_t st);

}  // namespace gnf
