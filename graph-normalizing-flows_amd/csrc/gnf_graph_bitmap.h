// What the graph scores (gnf_graph_stats / _orbits / _spectra / _components / _hashes .hip) share: the 64-bit adjacency bitmap of
// a batch read as undirected simple graphs (one word per (node, 64 graph-local columns); the layout is described in
// gnf_graph_stats.hip, gnf_graph_bitmap.hip builds it), the graph-range helpers, the row preamble, the per-node degree and
// triangle walk, the wave sums, the grid cap and the host-side check of csr and max_nodes_per_graph.
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

// Zeroes the bitmap of a validated batch with nodes (n > 0, b > 0) on the stream and fills it and gid (k_stats_bitmap,
// gnf_graph_bitmap.hip); bitmap [N][W] and gid [N] are the two arrays of a StatsWs, W = ceil(cap / 64).
int build_graph_bitmap(const GnfCsr* csr, int32_t cap, int64_t W, unsigned long long* bitmap, int32_t* gid, hipStream_t st);

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
template <class Off>   // int32 node_offsets of a GnfCsr, or the int64 ones the decoders scan
__device__ __forceinline__ void stats_graph_range(const Off* __restrict__ off, int g, int64_t n_nodes, int max_nodes,
                                                  int64_t& n0, int& ng) {
    n0 = off[g];
    int64_t n1 = off[g + 1];
    if (n0 < 0) n0 = 0;
    if (n1 > n_nodes) n1 = n_nodes;
    int64_t c = n1 - n0;
    if (c > max_nodes) c = max_nodes;
    ng = c > 0 ? (int)c : 0;
}

// the graph of bitmap row i and its window; false for a row in no graph or past the bound inside its graph (g, n0, ng are then
// not to be used).  gid is written by k_stats_bitmap alone: -1 or a graph of the batch.
__device__ __forceinline__ bool graph_of_row(const int32_t* __restrict__ off, const int32_t* __restrict__ gid, int64_t n_nodes,
                                             int max_nodes, int64_t i, int& g, int64_t& n0, int& ng) {
    g = gid[i];
    if (g < 0) return false;
    stats_graph_range(off, g, n_nodes, max_nodes, n0, ng);
    const int64_t li = i - n0;
    return li >= 0 && li < ng;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return __shfl(v, 0, 64);
}

// Hands the set bits of the LDS row to the lanes 64 at a time through the 128-entry LDS queue: a node of any degree keeps the
// wave full.  One wave per workgroup; visit(lj) runs once per neighbour lj.
template <class Visit>
__device__ __forceinline__ void for_each_neighbour(const unsigned long long* row, int32_t* queue, int words, int lane,
                                                   Visit visit) {
    int q = 0;   // entries waiting in the queue (< 64 between words)
    for (int w = 0; w < words; ++w) {
        const unsigned long long word = row[w];
        if (word == 0) continue;
        if ((word >> lane) & 1ull) queue[q + __popcll(word & ((1ull << lane) - 1ull))] = w * 64 + lane;
        q += __popcll(word);
        __syncthreads();
        if (q >= 64) {
            visit(queue[lane]);
            const int32_t tail = queue[64 + lane];
            __syncthreads();
            q -= 64;
            if (lane < q) queue[lane] = tail;
            __syncthreads();
        }
    }
    if (lane < q) visit(queue[lane]);
}

// Degree d and triangle count t of bitmap row i (graph window n0, `words` words), by the one wave of a workgroup; every lane
// gets both.  Loads the row into LDS (row [W] words, queue [128] graph-local neighbour ids) and leaves it there:
// d = sum_w popc(row_i[w]), t = 1/2 sum_{j in N(i)} sum_w popc(row_i[w] & row_j[w]), lane = one neighbour j reading row_j from
// global memory.
__device__ __forceinline__ void row_degree_triangles(const unsigned long long* __restrict__ bitmap, int64_t i,
                                                     unsigned long long* row, int32_t* queue, int words, int64_t n0, int64_t W,
                                                     unsigned long long& d, unsigned long long& t) {
    const int lane = threadIdx.x;
    __syncthreads();   // the previous node's readers are done
    d = 0;
    for (int w = lane; w < words; w += 64) {
        const unsigned long long v = bitmap[i * W + w];
        row[w] = v;
        d += __popcll(v);
    }
    __syncthreads();
    d = wave_sum_u64(d);
    unsigned long long acc = 0;   // common neighbours of i and the neighbour a lane holds
    for_each_neighbour(row, queue, words, lane, [&](int lj) {
        const unsigned long long* rj = bitmap + (n0 + lj) * W;
        for (int w = 0; w < words; ++w) acc += __popcll(row[w] & rj[w]);
    });
    t = wave_sum_u64(acc) >> 1;
}

inline unsigned stats_grid(int64_t items) {
    if (items < 1) items = 1;
    return (unsigned)(items > kStatsGridMax ? kStatsGridMax : items);
}

// what every batch entry point on the bitmap asks of csr and max_nodes_per_graph (host only; `limit` is the entry point's
// largest bound, `why` the reason for it).  n_nodes above INT32_MAX is the caller's to refuse where node ids are held in int32.
inline int graph_csr_ok(const char* what, const GnfCsr* csr, int32_t cap, int32_t limit, const char* why) {
    if (!csr) {
        set_error("%s: null csr", what);
        return GNF_EINVAL;
    }
    if (cap < 0 || cap > limit) {
        set_error("%s: max_nodes_per_graph=%d (0 <= max_nodes_per_graph <= %d: %s)", what, cap, limit, why);
        return GNF_ESHAPE;
    }
    if (csr->n_nodes < 0 || csr->n_edges < 0 || csr->n_graphs < 0 || csr->n_graphs > 0x7fffffff) {
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
