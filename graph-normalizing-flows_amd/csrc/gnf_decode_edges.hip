// Sampled embeddings -> edge lists on the device: what the reference does on the host after pred_adj
// (generate_graphs.py:68-78, train_grevnet_with_data.py:532-540: `pred_adj > 0.5`, one adjacency block per
// graph).  Edge (sender = j, receiver = i) of graph g exists iff P[i, j] > threshold, P as k_pred_adj computes it
// (gnf_decode.hip; loss.py:45-53,154-159) - the SAME fp32 expression, term for term, so that the edge set is bit-equal to
// `pred_adj(...) > threshold`; the diagonal is an edge only with self_loops, and then always.  The dense [n_g, n_g] float
// blocks are never written: pass 1 leaves one 64-bit ballot word per (row, 64 columns) and a count per row, a scan turns
// the counts into rowptr / n_edge / total, pass 2 expands the bitmap into (senders, receivers), receivers ascending and
// senders ascending within a receiver - (rowptr, senders) IS the receiver-sorted CSR of the edge list, and because
// d2(i, j) and d2(j, i) are the same fp32 number the edge set is symmetric, so it is the by-sender CSR as well.
// No atomics: every word, count and edge has exactly one writer.
// gnf_adj_edges_count_dist_f32 (include/gnf_distance.h) is pass 1 with another DistSigmoid (gnf_distance_dev.h).
// The workspace layout, the grid and the size rules are gnf_edge_ws.h's, shared with gnf_random_graphs.hip, whose kernels are
// another pass 1 in front of the same scan and the same pass 2.
#include "gnf_distance_dev.h"
#include "gnf_edge_ws.h"
#include "gnf_graph_bitmap.h"

namespace gnf {

// A graph's rows come from stats_graph_range (gnf_graph_bitmap.h), cut to the node buffer and to the `max_nodes` columns the
// bitmap holds: counts that do not describe the batch (or a bound below the largest graph) lose edges, they never reach
// outside the arrays.

// pass 1.  One workgroup per (graph, 16-row tile), the tile's rows in LDS as in k_pred_adj; wave w owns rows 4 w .. 4 w + 3
// of the tile and walks the graph's columns 64 at a time (lane = column): one read of z_j serves its four rows, one ballot
// per row is the bitmap word, and the wave adds up its rows' popcounts in registers.
template <bool LDS_ROWS>
__global__ __launch_bounds__(256) void k_edge_count(const float* __restrict__ z, int64_t ld, int D,
                                                    const int64_t* __restrict__ node_off, int64_t n_nodes, int max_nodes,
                                                    int64_t W, float threshold, int self_loops, DistSigmoid dist_arg,
                                                    unsigned long long* __restrict__ bitmap, int32_t* __restrict__ rowcnt) {
    extern __shared__ float zi[];  // [kEdgeTile][D]
    int64_t n0;
    int ng;
    stats_graph_range(node_off, blockIdx.x, n_nodes, max_nodes, n0, ng);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int words = (ng + 63) / 64;
    const DistSigmoid dist = dist_arg.load();   // (device-resident parameters: once per workgroup)
    for (int i0 = blockIdx.y * kEdgeTile; i0 < ng; i0 += gridDim.y * kEdgeTile) {   // (uniform over the workgroup)
        const int rows = ng - i0 < kEdgeTile ? ng - i0 : kEdgeTile;
        if constexpr (LDS_ROWS) {
            __syncthreads();   // the previous tile's readers are done
            stage_row_tile(zi, z, ld, D, n0 + i0, rows);
            __syncthreads();
        }
        const int r0 = wave * kEdgeWaveRows;
        if (r0 >= rows) continue;
        const float* zr[kEdgeWaveRows];
        int cnt[kEdgeWaveRows];
        for (int q = 0; q < kEdgeWaveRows; ++q) {
            const int rl = r0 + q < rows ? r0 + q : rows - 1;   // rows past the tile's end repeat its last row; not stored
            zr[q] = LDS_ROWS ? zi + rl * D : z + (n0 + i0 + rl) * ld;
            cnt[q] = 0;
        }
        for (int w = 0; w < words; ++w) {
            const int j = w * 64 + lane;
            const bool col = j < ng;
            const float* zj = z + (n0 + (col ? j : ng - 1)) * ld;
            float d2[kEdgeWaveRows];
            pair_d2(zr, zj, D, d2);
            for (int q = 0; q < kEdgeWaveRows; ++q) {
                const int i = i0 + r0 + q;
                const float a = dist.logit(d2[q]);
                const float p = 1.f / (1.f + expf(-a));
                const bool edge = col && (i == j ? self_loops != 0 : p > threshold);
                const unsigned long long word = __ballot(edge);
                if (r0 + q < rows) {
                    if (lane == 0) bitmap[(n0 + i) * W + w] = word;
                    cnt[q] += __popcll(word);
                }
            }
        }
        if (lane == 0)
            for (int q = 0; q < kEdgeWaveRows; ++q)
                if (r0 + q < rows) rowcnt[n0 + i0 + r0 + q] = cnt[q];
    }
}

// rowptr = exclusive prefix of rowcnt (one workgroup, a contiguous chunk of rows per lane: any N), then the per-graph edge
// counts and the total.  n_nodes * max_nodes <= INT32_MAX (checked on the host) bounds every sum.
__global__ __launch_bounds__(256) void k_edge_scan(const int32_t* __restrict__ rowcnt, int64_t n_nodes,
                                                   const int64_t* __restrict__ node_off, int64_t n_graphs,
                                                   int32_t* __restrict__ rowptr, int32_t* __restrict__ n_edge,
                                                   int64_t* __restrict__ total) {
    __shared__ int32_t sh[257];
    const int64_t chunk = (n_nodes + 255) / 256;
    const int64_t beg = (int64_t)threadIdx.x * chunk;
    int64_t end = beg + chunk;
    if (end > n_nodes) end = n_nodes;
    int32_t l = 0;
    for (int64_t i = beg; i < end; ++i) l += rowcnt[i];
    sh[threadIdx.x + 1] = l;
    if (threadIdx.x == 0) sh[0] = 0;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i <= 256; ++i) sh[i] += sh[i - 1];
    __syncthreads();
    int32_t r = sh[threadIdx.x];
    if (threadIdx.x == 0) {
        rowptr[0] = 0;
        *total = sh[256];
    }
    for (int64_t i = beg; i < end; ++i) {
        r += rowcnt[i];
        rowptr[i + 1] = r;
    }
    __syncthreads();   // rowptr written above is read below by other lanes of this workgroup
    for (int64_t g = threadIdx.x; g < n_graphs; g += 256) {
        int64_t a = node_off[g], b = node_off[g + 1];
        a = a < 0 ? 0 : (a > n_nodes ? n_nodes : a);
        b = b < a ? a : (b > n_nodes ? n_nodes : b);
        n_edge[g] = rowptr[b] - rowptr[a];
    }
}

// pass 2.  Same grid and row ownership as pass 1; a wave expands one row at a time: lane = column of the current word,
// edge id = rowptr[row] + (edges in the row's earlier words) + (set bits below the lane).  Ids >= edge_capacity are dropped.
__global__ __launch_bounds__(256) void k_edge_fill(const int64_t* __restrict__ node_off, int64_t n_nodes, int max_nodes,
                                                   int64_t W, const unsigned long long* __restrict__ bitmap,
                                                   const int32_t* __restrict__ rowptr, int64_t edge_capacity,
                                                   int32_t* __restrict__ senders, int32_t* __restrict__ receivers) {
    int64_t n0;
    int ng;
    stats_graph_range(node_off, blockIdx.x, n_nodes, max_nodes, n0, ng);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int words = (ng + 63) / 64;
    for (int i0 = blockIdx.y * kEdgeTile; i0 < ng; i0 += gridDim.y * kEdgeTile) {
        for (int q = 0; q < kEdgeWaveRows; ++q) {
            const int i = i0 + wave * kEdgeWaveRows + q;
            if (i >= ng) break;
            int64_t e0 = rowptr[n0 + i];
            for (int w = 0; w < words && e0 >= 0 && e0 < edge_capacity; ++w) {
                const unsigned long long word = bitmap[(n0 + i) * W + w];
                const int64_t e = e0 + __popcll(word & ((1ull << lane) - 1ull));
                if (((word >> lane) & 1ull) && e < edge_capacity) {
                    senders[e] = (int32_t)(n0 + w * 64 + lane);
                    receivers[e] = (int32_t)(n0 + i);
                }
                e0 += __popcll(word);
            }
        }
    }
}

int launch_edge_scan(const int32_t* rowcnt, int64_t n_nodes, const int64_t* node_off, int64_t n_graphs, int32_t* rowptr,
                     int32_t* n_edge, int64_t* total, hipStream_t st) {
    hipLaunchKernelGGL(k_edge_scan, dim3(1), dim3(256), 0, st, rowcnt, n_nodes, node_off, n_graphs, rowptr, n_edge, total);
    GNF_LAUNCH_CHECK("k_edge_scan");
    return GNF_OK;
}

// the two counting entry points: same checks, same launches
static int edges_count(const char* what, DistSigmoid dist, const float* z, int64_t ld, int32_t D, const int32_t* n_node,
                       int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph, float threshold, int32_t self_loops,
                       int32_t* rowptr, int32_t* n_edge, int64_t* total, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    if (D < 1 || ld < D) {
        set_error("%s: D=%d ld=%lld", what, D, (long long)ld);
        return GNF_ESHAPE;
    }
    if (int rc = edge_sizes_ok(what, n_graphs, n_nodes, max_nodes_per_graph)) return rc;
    if (n_graphs > 0x7fffffff) {
        set_error("%s: n_graphs=%lld", what, (long long)n_graphs);
        return GNF_ESHAPE;
    }
    if (!rowptr || !total || !ws || (n_graphs > 0 && (!n_node || !n_edge)) || (n_nodes > 0 && !z)) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const EdgeWs L = edge_ws(n_graphs, n_nodes, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    int64_t* node_off = (int64_t*)((char*)ws + L.node_off);
    unsigned long long* bitmap = (unsigned long long*)((char*)ws + L.bitmap);
    int32_t* rowcnt = (int32_t*)((char*)ws + L.rowcnt);
    if (int rc = launch_node_offsets(n_node, n_graphs, node_off, nullptr, st)) return rc;
    if (n_graphs > 0 && n_nodes > 0) {
        const dim3 grid = edge_grid(n_graphs, max_nodes_per_graph);
        const size_t row_tile = (size_t)kEdgeTile * D * sizeof(float);
        if (row_tile <= 64 * 1024)
            hipLaunchKernelGGL(k_edge_count<true>, grid, dim3(256), row_tile, st, z, ld, D, node_off, n_nodes,
                               max_nodes_per_graph, L.W, threshold, self_loops, dist, bitmap, rowcnt);
        else
            hipLaunchKernelGGL(k_edge_count<false>, grid, dim3(256), 0, st, z, ld, D, node_off, n_nodes,
                               max_nodes_per_graph, L.W, threshold, self_loops, dist, bitmap, rowcnt);
        GNF_LAUNCH_CHECK("k_edge_count");
    }
    return launch_edge_scan(rowcnt, n_graphs > 0 ? n_nodes : 0, node_off, n_graphs, rowptr, n_edge, total, st);
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_adj_edges_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_nodes < 0 || max_nodes_per_graph < 0) return 0;
    return edge_ws(n_graphs, n_nodes, max_nodes_per_graph).total;
}

int gnf_adj_edges_count_f32(const float* z, int64_t ld, int32_t D, const int32_t* n_node, int64_t n_graphs, int64_t n_nodes,
                            int32_t max_nodes_per_graph, float threshold, int32_t self_loops, int32_t* rowptr,
                            int32_t* n_edge, int64_t* total, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    return edges_count("gnf_adj_edges_count_f32", dist_scaled_hacky(D), z, ld, D, n_node,
                       n_graphs, n_nodes, max_nodes_per_graph, threshold, self_loops, rowptr, n_edge, total, ws, ws_bytes,
                       stream);
}

int gnf_adj_edges_count_dist_f32(const GnfDistance* dist, const float* z, int64_t ld, int32_t D, const int32_t* n_node,
                                 int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph, float threshold,
                                 int32_t self_loops, int32_t* rowptr, int32_t* n_edge, int64_t* total, void* ws, size_t ws_bytes,
                                 gnf_stream_t stream) {
    if (!dist) {
        set_error("gnf_adj_edges_count_dist_f32: null dist");
        return GNF_EINVAL;
    }
    return edges_count("gnf_adj_edges_count_dist_f32", dist_sigmoid(*dist, D), z, ld, D, n_node, n_graphs,
                       n_nodes, max_nodes_per_graph, threshold, self_loops, rowptr, n_edge, total, ws, ws_bytes, stream);
}

int gnf_adj_edges_fill(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph, const int32_t* rowptr,
                       int64_t edge_capacity, int32_t* senders, int32_t* receivers, const void* ws, size_t ws_bytes,
                       gnf_stream_t stream) {
    const char* what = "gnf_adj_edges_fill";
    if (int rc = edge_sizes_ok(what, n_graphs, n_nodes, max_nodes_per_graph)) return rc;
    if (edge_capacity < 0 || n_graphs > 0x7fffffff) {
        set_error("%s: edge_capacity=%lld n_graphs=%lld", what, (long long)edge_capacity, (long long)n_graphs);
        return GNF_ESHAPE;
    }
    if (!rowptr || !ws || (edge_capacity > 0 && (!senders || !receivers))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const EdgeWs L = edge_ws(n_graphs, n_nodes, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    if (n_graphs == 0 || n_nodes == 0 || edge_capacity == 0) return GNF_OK;
    hipLaunchKernelGGL(k_edge_fill, edge_grid(n_graphs, max_nodes_per_graph), dim3(256), 0, (hipStream_t)stream,
                       (const int64_t*)((const char*)ws + L.node_off), n_nodes, max_nodes_per_graph, L.W,
                       (const unsigned long long*)((const char*)ws + L.bitmap), rowptr, edge_capacity, senders, receivers);
    GNF_LAUNCH_CHECK("k_edge_fill");
    return GNF_OK;
}

}  // extern "C"
