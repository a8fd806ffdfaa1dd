// Device helpers of the graph-scope attention kernels (GnfAttn.scope == GNF_ATTN_GRAPH: gnf_attn_graph.hip,
// gnf_attn_graph_bwd.hip).  A node attends to every node of its own graph, itself included; the graph of node r is the
// g with node_offsets[g] <= r < node_offsets[g + 1].  Every range below is clamped to [0, n): offsets that do not describe
// the batch give wrong numbers, never an access outside the node arrays.
#pragma once
#include "gnf_attn_core_dev.h"

namespace gnf {

struct GraphAttnWin {
    const int32_t* off;  // [n_graphs + 1]
    int32_t n_graphs, n;
};

// the largest g in [0, n_graphs) with off[g] <= r (empty graphs share their offset with the next one: the last of equal
// offsets is the graph that holds r)
__device__ __forceinline__ int graph_attn_graph_of(const GraphAttnWin& w, int r) {
    int lo = 0, hi = w.n_graphs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (w.off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int graph_attn_clamp(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }

// node range [lo, hi) of r's graph
__device__ __forceinline__ void graph_attn_range(const GraphAttnWin& w, int r, int& lo, int& hi) {
    const int g = graph_attn_graph_of(w, r);
    lo = graph_attn_clamp(w.off[g], w.n);
    hi = graph_attn_clamp(w.off[g + 1], w.n);
}

// the window of a tile of rows [row0, row0 + rows): from the first row's graph start to the last live row's graph end
__device__ __forceinline__ void graph_attn_tile_window(const GraphAttnWin& w, int row0, int rows, int& lo, int& hi) {
    const int last = row0 + rows - 1 < w.n - 1 ? row0 + rows - 1 : w.n - 1;
    int l0, h0, l1, h1;
    graph_attn_range(w, row0, l0, h0);
    graph_attn_range(w, last, l1, h1);
    lo = l0 < l1 ? l0 : l1;
    hi = h1 > h0 ? h1 : h0;
    if (hi < lo) hi = lo;
}

}  // namespace gnf
