// Per-graph log-likelihood terms of a batch (gnf_grevnet_per_graph_f32): the reduction that follows the flow's last
// half-step.  A batch is a block-diagonal union of graphs and log|det| is a plain sum over nodes, so graph g's share is
//   logdet_g = sum_{r in g} sum_{half-steps} sum_j s[r, j]  +  n_g * sum_{bijectors} c        (c: gnf_bn.hip, per node)
//   sumsq_g  = sum_{r in g} sum_j z[r, j]^2
// The half-step kernels' ROWLD instances left sum_j s[r, j] per row and half-step (one slot of n doubles each, plain
// stores by the workgroup that owns the row); here one wave or one workgroup per graph adds them up in fp64 in a fixed
// order: a thread's rows / elements strided by the group size, lanes by shuffles, waves in wave order.  No atomics: two
// runs give the same bits.  The reference has no counterpart: its loss needs the batch scalar only (gnn.py:322,337).
#include "gnf_common.h"

namespace gnf {

// TPG threads per graph: 64 (four graphs per workgroup; batches of small graphs) or 256 (one graph per workgroup)
template <int TPG>
__global__ __launch_bounds__(256) void k_per_graph(const double* __restrict__ row_ld, int n_slots, int64_t n,
                                                   const double* __restrict__ bn_c, int n_c, const float* __restrict__ z,
                                                   int64_t ld, int D, const int32_t* __restrict__ node_offsets,
                                                   int64_t n_graphs, double* __restrict__ graph_out) {
    __shared__ double sh[2][4];
    const int tid = threadIdx.x;
    const int l = tid % TPG;
    const int64_t g = (int64_t)blockIdx.x * (256 / TPG) + tid / TPG;
    const bool live = g < n_graphs;
    // offsets that do not describe the batch give wrong numbers, never an access outside the node arrays
    int64_t lo = live ? (int64_t)node_offsets[g] : 0, hi = live ? (int64_t)node_offsets[g + 1] : 0;
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
    const int64_t ng = hi - lo;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t r = lo + l; r < hi; r += TPG) {
        double v = 0.0;
        for (int k = 0; k < n_slots; ++k) v += row_ld[(int64_t)k * n + r];  // half-step order
        a0 += v;
    }
    const int64_t total = ng * D;
    for (int64_t i = l; i < total; i += TPG) {
        const int64_t r = i / D;
        const int f = (int)(i - r * D);
        const double v = (double)z[(lo + r) * ld + f];
        a1 += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_down(a0, off, 64);
        a1 += __shfl_down(a1, off, 64);
    }
    if (TPG == 256) {
        if ((tid & 63) == 0) sh[0][tid >> 6] = a0, sh[1][tid >> 6] = a1;
        __syncthreads();
        a0 = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        a1 = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    }
    if (live && l == 0) {
        double c = 0.0;
        for (int k = 0; k < n_c; ++k) c += bn_c[k];
        graph_out[2 * g + 0] = a0 + (double)ng * c;
        graph_out[2 * g + 1] = a1;
    }
}

int launch_per_graph(const double* row_ld, int n_slots, int64_t n, const double* bn_c, int n_c, const float* z, int64_t ld,
                     int32_t D, const int32_t* node_offsets, int64_t n_graphs, double* graph_out, hipStream_t st) {
    if (n_graphs <= 0) return GNF_OK;
    if (n <= 16 * n_graphs) {  // sixteen nodes per graph or fewer on average: a wave per graph
        const int64_t blocks = (n_graphs + 3) / 4;
        hipLaunchKernelGGL(k_per_graph<64>, dim3((unsigned)blocks), dim3(256), 0, st, row_ld, n_slots, n, bn_c, n_c, z, ld, D,
                           node_offsets, n_graphs, graph_out);
    } else {
        hipLaunchKernelGGL(k_per_graph<256>, dim3((unsigned)n_graphs), dim3(256), 0, st, row_ld, n_slots, n, bn_c, n_c, z, ld, D,
                           node_offsets, n_graphs, graph_out);
    }
    GNF_LAUNCH_CHECK("k_per_graph");
    return GNF_OK;
}

}  // namespace gnf
