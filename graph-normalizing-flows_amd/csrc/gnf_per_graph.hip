// Per-graph log-likelihood terms of a batch (gnf_grevnet_per_graph_f32): the reduction that follows the flow's last
// half-step.  A batch is a block-diagonal union of graphs and log|det| is a plain sum over nodes, so graph g's share is
//   logdet_g = sum_{r in g} sum_{half-steps} sum_j s[r, j]  +  n_g * sum_{bijectors} c        (c: gnf_bn.hip, per node)
//   sumsq_g  = sum_{r in g} sum_j z[r, j]^2
// The half-step kernels' ROWLD instances left sum_j s[r, j] per row and half-step (one slot of n doubles each, plain
// stores by the workgroup that owns the row); here one wave or one workgroup per graph adds them up in fp64 in a fixed
// order: a thread's rows / elements strided by the group size, lanes by shuffles, waves in wave order.  No atomics: two
// runs give the same bits.  The reference has no counterpart: its loss needs the batch scalar only (gnn.py:322,337).
// Below it, the same for the sampling direction (gnf_grevnet_inverse_per_graph_f32): the bijectors' constant terms, the
// reduction with the inverse's signs and sum z^2 of the source rows, and the batch sums in graph order.
#include "gnf_common.h"

namespace gnf {

// TPG threads per graph: 64 (four graphs per workgroup; batches of small graphs) or 256 (one graph per workgroup)
// INVERSE (gnf_grevnet_inverse_per_graph_f32, below): the rows hold + sum s of x = g(z), so the sign is applied here, once, and
// z is the walk's SOURCE.  row_ld == NULL: the launch in front of an in-place walk - only graph_out[2 g + 1]; z == NULL: the
// launch behind that walk - only graph_out[2 g + 0]; both: out of place, both entries.  Same ownership, same order of additions.
template <int TPG, bool INVERSE = false>
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
    for (int64_t r = lo + l; r < hi && (!INVERSE || row_ld); r += TPG) {
        double v = 0.0;
        for (int k = 0; k < n_slots; ++k) v += row_ld[(int64_t)k * n + r];  // half-step order
        a0 += v;
    }
    const int64_t total = !INVERSE || z ? ng * D : 0;
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
        if constexpr (INVERSE) {
            if (row_ld) graph_out[2 * g + 0] = (double)ng * c - a0;
            if (z) graph_out[2 * g + 1] = a1;
        } else {
            graph_out[2 * g + 0] = a0 + (double)ng * c;
            graph_out[2 * g + 1] = a1;
        }
    }
}

int launch_per_graph(const double* row_ld, int n_slots, int64_t n, const double* bn_c, int n_c, const float* z, int64_t ld,
                     int32_t D, const int32_t* node_offsets, int64_t n_graphs, double* graph_out, hipStream_t st, bool inverse) {
    if (n_graphs <= 0) return GNF_OK;
    const bool wave = n <= 16 * n_graphs;  // sixteen nodes per graph or fewer on average: a wave per graph
    const dim3 grid((unsigned)(wave ? (n_graphs + 3) / 4 : n_graphs));
#define GNF_PER_GRAPH(TPG_, INV_)                                                                                              \
    hipLaunchKernelGGL((k_per_graph<TPG_, INV_>), grid, dim3(256), 0, st, row_ld, n_slots, n, bn_c, n_c, z, ld, D, node_offsets, \
                       n_graphs, graph_out)
    if (inverse) {
        if (wave) GNF_PER_GRAPH(64, true); else GNF_PER_GRAPH(256, true);
    } else {
        if (wave) GNF_PER_GRAPH(64, false); else GNF_PER_GRAPH(256, false);
    }
#undef GNF_PER_GRAPH
    GNF_LAUNCH_CHECK("k_per_graph");
    return GNF_OK;
}

// ---- the sampling direction (gnf_grevnet_inverse_per_graph_f32) --------------------------------------------------------
// x = g(z): the half-step kernels' ROWLD instances leave + sum_j s[r, j] of the s each inverse coupling used, and
//   logdet_g = - sum_{r in g} sum_{half-steps} sum_j s[r, j]  +  n_g * sum_{bijectors} c,   c = sum_f (0.5 log(mvar_f + eps) - log gamma_f)
//   sumsq_g  = sum_{r in g} sum_j z[r, j]^2        of the INPUT rows
// The bijectors of g use constants, so c is a property of the flow: one small launch computes the 2T of them.

struct BnInvTerms {  // bijector k of this launch: device fp32 [H] each
    static constexpr int kMax = 32;
    const float* gamma[kMax];
    const float* mvar[kMax];
    float eps[kMax];
};
// a workgroup per bijector: the H terms in fp64 from the fp32 parameters (256 at a time, through LDS), added in feature order
__global__ __launch_bounds__(256) void k_bn_inverse_terms(const BnInvTerms t, int H, double* __restrict__ out) {
    __shared__ double term[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ gamma = t.gamma[k];
    const float* __restrict__ mvar = t.mvar[k];
    const double eps = (double)t.eps[k];
    double acc = 0.0;
    for (int f0 = 0; f0 < H; f0 += 256) {
        const int f = f0 + tid;
        if (f < H) term[tid] = 0.5 * log((double)mvar[f] + eps) - log((double)gamma[f]);
        __syncthreads();
        if (tid == 0) {
            const int w = H - f0 < 256 ? H - f0 : 256;
            for (int i = 0; i < w; ++i) acc += term[i];
        }
        __syncthreads();
    }
    if (tid == 0) out[k] = acc;
}

int launch_bn_inverse_terms(const GnfFlow* flow, int32_t H, double* bn_c, hipStream_t st) {
    const int T = flow->num_timesteps;
    // bn_c[idx], idx = 2 i + half: the slot order of the row sums (GnfFlow.bns is indexed half * T + i)
    for (int k0 = 0; k0 < 2 * T; k0 += BnInvTerms::kMax) {
        BnInvTerms t{};
        const int cnt = 2 * T - k0 < BnInvTerms::kMax ? 2 * T - k0 : BnInvTerms::kMax;
        for (int k = 0; k < cnt; ++k) {
            const int idx = k0 + k;
            const GnfBatchNorm* bn = &flow->bns[(idx & 1) * T + (idx >> 1)];
            t.gamma[k] = bn->gamma, t.mvar[k] = bn->moving_variance, t.eps[k] = bn->epsilon;
        }
        hipLaunchKernelGGL(k_bn_inverse_terms, dim3((unsigned)cnt), dim3(256), 0, st, t, H, bn_c + k0);
        GNF_LAUNCH_CHECK("k_bn_inverse_terms");
    }
    return GNF_OK;
}

// sums[k] = graph_out[0][k] + graph_out[1][k] + ... in graph order (what a sequential host loop gives): the workgroup
// stages 256 graphs at a time in LDS, thread k adds column k
__global__ __launch_bounds__(256) void k_graph_sums(const double* __restrict__ graph_out, int64_t n_graphs, double* __restrict__ sums) {
    __shared__ double st[512];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t g0 = 0; g0 < n_graphs; g0 += 256) {
        const int w = n_graphs - g0 < 256 ? (int)(n_graphs - g0) : 256;
        for (int i = tid; i < 2 * w; i += 256) st[i] = graph_out[2 * g0 + i];
        __syncthreads();
        if (tid < 2)
            for (int i = 0; i < w; ++i) acc += st[2 * i + tid];
        __syncthreads();
    }
    if (tid < 2) sums[tid] = acc;
}

int launch_graph_sums(const double* graph_out, int64_t n_graphs, double* sums, hipStream_t st) {
    hipLaunchKernelGGL(k_graph_sums, dim3(1), dim3(256), 0, st, graph_out, n_graphs, sums);
    GNF_LAUNCH_CHECK("k_graph_sums");
    return GNF_OK;
}

}  // namespace gnf
