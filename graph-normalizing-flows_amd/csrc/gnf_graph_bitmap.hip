// The adjacency bitmap every graph score starts from (layout and graph model: gnf_graph_stats.hip): the one kernel that fills it
// and the one host function that launches it, build_graph_bitmap (declared in gnf_graph_bitmap.h).
#include "gnf_graph_bitmap.h"

namespace gnf {

// one wave per CSR row i sets bit (i, j - n0) and bit (j, i - n0) of the zeroed bitmap for every entry (receiver i, sender j),
// i != j, and writes gid[i]; lanes take the row's entries 64 at a time.  An entry whose endpoints are not both inside the
// graph's [n0, n0 + ng) window is dropped (never an access outside the bitmap).  Grid stats_grid((n_nodes + 3) / 4), 256 threads
__global__ __launch_bounds__(256) void k_stats_bitmap(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      int64_t n_nodes, int64_t n_edges, const int32_t* __restrict__ off,
                                                      int64_t n_graphs, int max_nodes, int64_t W,
                                                      unsigned long long* __restrict__ bitmap, int32_t* __restrict__ gid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_nodes; i += (int64_t)gridDim.x * 4) {
        const int g = stats_graph_of(off, n_graphs, i);
        if (lane == 0) gid[i] = g;
        if (g < 0) continue;
        int64_t n0;
        int ng;
        stats_graph_range(off, g, n_nodes, max_nodes, n0, ng);
        const int64_t li = i - n0;
        if (li < 0 || li >= ng) continue;
        int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > n_edges) e1 = n_edges;
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int64_t lj = (int64_t)col[e] - n0;
            if (lj < 0 || lj >= ng || lj == li) continue;
            atomicOr(&bitmap[i * W + (lj >> 6)], 1ull << (lj & 63));
            atomicOr(&bitmap[(n0 + lj) * W + (li >> 6)], 1ull << (li & 63));
        }
    }
}

int build_graph_bitmap(const GnfCsr* csr, int32_t cap, int64_t W, unsigned long long* bitmap, int32_t* gid, hipStream_t st) {
    const int64_t n = csr->n_nodes;
    GNF_HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)n * (size_t)W * sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_stats_bitmap, dim3(stats_grid((n + 3) / 4)), dim3(256), 0, st, csr->rowptr, csr->col, n, csr->n_edges,
                       csr->node_offsets, csr->n_graphs, cap, W, bitmap, gid);
    GNF_LAUNCH_CHECK("k_stats_bitmap");
    return GNF_OK;
}

}  // namespace gnf
