// Scoring generated graphs on the device: per-node degree / triangle counts, per-graph degree and clustering-coefficient
// histograms, and the MMD of two histogram sets - the evaluation GraphRNN-style papers report (MMD of degree and clustering
// histograms against held-out graphs).  The reference stops at pickling the graphs (generate_graphs.py:68-84); nothing in it
// corresponds to these kernels.
//
// Graph model.  Every graph is read as UNDIRECTED and SIMPLE whatever its edge list looks like: self loops are ignored,
// duplicate edges count once, an edge present in one direction only counts in both, and the order of the senders inside a
// CSR row does not matter.  That is what the adjacency bitmap gives for free: one 64-bit word per (node, 64 graph-local
// columns) - the decoder's shape (gnf_decode_edges.hip) - zeroed on the stream, then for every CSR entry (receiver i,
// sender j), i != j, bit (i, j - n0) and bit (j, i - n0) are set with a global 64-bit atomicOr (build_graph_bitmap,
// gnf_graph_bitmap.hip).  OR is order-independent: the bitmap, and everything below, is deterministic.
//
// Per node (one wave, one workgroup; row_degree_triangles, gnf_graph_bitmap.h): deg_i = sum_w popc(row_i[w]);
// tri_i = 1/2 sum_{j in N(i)} sum_w popc(row_i[w] & row_j[w]).
// row_i sits in LDS; the set bits of the row are compacted into a 128-entry LDS queue and handed out to the lanes 64 at a time
// (lane = one neighbour j, reading row_j from global memory), so a node of any degree keeps the wave full.
//
// Clustering bin, exact integer arithmetic in 64 bits - NORMATIVE:  d < 2 -> bin 0;  else min(bins - 1, (2 T bins) / (d (d - 1))).
// This is floor(c * bins) on the exact rational c = 2 T / (d (d - 1)) with c = 1 landing in the last bin.  Where
// numpy.histogram's float rounding of a bin edge (c = 0.1 with 100 bins: 0.1 * 100 in floating point) disagrees with it, this
// definition wins.
//
// Histogram MMD.  Sets A [a][La] and B [b][Lb] of int32 histograms, the narrower read as zero-padded to L = max(La, Lb); every
// row is normalised to a pmf in fp64, rows with sum <= 0 (a graph without nodes) are excluded and counted out.  For every
// unordered pair (p <= q) of the concatenated set one wave computes
//   GNF_MMD_GAUSSIAN_EMD: W = (1 / distance_scaling) sum_{k=0}^{L-2} |sum_{i<=k} (x_i - y_i)|   (1-D earth mover's distance,
//                         unit bin spacing; wave prefix scan over 64-bin chunks with a carry)
//   GNF_MMD_GAUSSIAN_TV:  W = 1/2 sum_i |x_i - y_i|
// and k = exp(-W^2 / (2 sigma^2)), added to the AA / BB / AB block sum (diagonal pairs once, off-diagonal pairs inside a block
// twice, cross pairs once).  No floating-point atomics: workgroup p owns row p's pairs and leaves one fp64 partial triple in the
// workspace, a single workgroup adds the partials up in a fixed order - two calls give the same bits.
#include "gnf_graph_bitmap.h"

namespace gnf {

static constexpr int kStatsMaxNodes = 65536;   // tri_i <= C(n - 1, 2) must fit int32

// one wave = one workgroup per node.  LDS: row_i [W] words | queue [128] graph-local neighbour ids.
__global__ __launch_bounds__(64) void k_stats_nodes(const int32_t* __restrict__ off, int64_t n_nodes, int max_nodes, int64_t W,
                                                    int bins, const unsigned long long* __restrict__ bitmap,
                                                    const int32_t* __restrict__ gid, int32_t* __restrict__ degree,
                                                    int32_t* __restrict__ triangles, int32_t* __restrict__ degree_hist,
                                                    int32_t* __restrict__ clustering_hist,
                                                    unsigned long long* __restrict__ deg_sum,
                                                    unsigned long long* __restrict__ tri_sum) {
    extern __shared__ unsigned long long stats_lds[];
    unsigned long long* row = stats_lds;        // [W]
    int32_t* queue = (int32_t*)(stats_lds + W);  // [128]
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < n_nodes; i += gridDim.x) {   // (uniform over the workgroup)
        int g, ng;
        int64_t n0;
        if (!graph_of_row(off, gid, n_nodes, max_nodes, i, g, n0, ng)) {   // the caller's error: zeros, no histogram entry
            if (lane == 0) {
                degree[i] = 0;
                triangles[i] = 0;
            }
            continue;
        }
        unsigned long long d, t;
        row_degree_triangles(bitmap, i, row, queue, (ng + 63) / 64, n0, W, d, t);
        if (lane == 0) {
            degree[i] = (int32_t)d;
            triangles[i] = (int32_t)t;
            unsigned long long bin = 0;
            if (d >= 2) {
                bin = (2ull * t * (unsigned long long)bins) / (d * (d - 1ull));
                if (bin > (unsigned long long)(bins - 1)) bin = bins - 1;
            }
            atomicAdd(&degree_hist[(int64_t)g * max_nodes + (int64_t)d], 1);   // d <= ng - 1 < max_nodes
            atomicAdd(&clustering_hist[(int64_t)g * bins + (int64_t)bin], 1);
            atomicAdd(&deg_sum[g], d);
            atomicAdd(&tri_sum[g], t);
        }
    }
}

// n_edges = sum deg / 2, n_triangles = sum tri / 3 (the sums were accumulated in place)
__global__ __launch_bounds__(256) void k_stats_finish(int64_t n_graphs, int64_t* __restrict__ n_edges,
                                                      int64_t* __restrict__ n_triangles) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_graphs; g += (int64_t)gridDim.x * 256) {
        n_edges[g] /= 2;
        n_triangles[g] /= 3;
    }
}

// ---- histogram MMD ---------------------------------------------------------------------------------------------------------
// workspace (host only): inv double [a + b] (1 / row sum, 0 = excluded) | partials double [a + b][3]
struct MmdSets {
    const int32_t *ha, *hb;
    int64_t a, b, lda, ldb;
    int32_t La, Lb;
};
__device__ __forceinline__ const int32_t* mmd_row(const MmdSets& s, int64_t r, int& len) {
    if (r < s.a) {
        len = s.La;
        return s.ha + r * s.lda;
    }
    len = s.Lb;
    return s.hb + (r - s.a) * s.ldb;
}

__global__ __launch_bounds__(256) void k_mmd_rowsums(MmdSets s, double* __restrict__ inv) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = s.a + s.b;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        int len;
        const int32_t* h = mmd_row(s, r, len);
        long long sum = 0;
        for (int i = lane; i < len; i += 64) sum += h[i];
        sum = (long long)wave_sum_u64((unsigned long long)sum);
        if (lane == 0) inv[r] = sum > 0 ? 1.0 / (double)sum : 0.0;
    }
}

// workgroup p: the pairs (p, q), q >= p; wave w takes q = p + w, p + w + 4, ...
__global__ __launch_bounds__(256) void k_mmd_pairs(MmdSets s, int emd, double inv_scaling, double neg_half_inv_sigma2,
                                                   const double* __restrict__ inv, double* __restrict__ partials) {
    __shared__ double sh[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = s.a + s.b, p = blockIdx.x;
    const int L = s.La > s.Lb ? s.La : s.Lb;
    int lp;
    const int32_t* hp = mmd_row(s, p, lp);
    const double ip = inv[p];
    double acc[3] = {0.0, 0.0, 0.0};   // AA, BB, AB
    if (ip > 0.0) {
        for (int64_t q = p + wave; q < n; q += 4) {
            const double iq = inv[q];
            if (!(iq > 0.0)) continue;
            int lq;
            const int32_t* hq = mmd_row(s, q, lq);
            double part = 0.0, carry = 0.0;
            for (int c0 = 0; c0 < L; c0 += 64) {
                const int i = c0 + lane;
                const double x = i < lp ? (double)hp[i] * ip : 0.0;
                const double y = i < lq ? (double)hq[i] * iq : 0.0;
                double v = x - y;
                if (emd) {
                    for (int o = 1; o < 64; o <<= 1) {   // inclusive prefix sum of the chunk
                        const double u = __shfl_up(v, o, 64);
                        if (lane >= o) v += u;
                    }
                    v += carry;
                    carry = __shfl(v, 63, 64);
                    if (i < L - 1) part += fabs(v);
                } else {
                    part += fabs(v);   // (i >= L: x = y = 0)
                }
            }
            const double wdist = wave_sum_f64(part) * (emd ? inv_scaling : 0.5);
            const double k = exp(wdist * wdist * neg_half_inv_sigma2);
            const int slot = q < s.a ? 0 : (p >= s.a ? 1 : 2);
            acc[slot] += (slot != 2 && q != p) ? 2.0 * k : k;
        }
    }
    if (lane == 0)
        for (int c = 0; c < 3; ++c) sh[wave][c] = acc[c];
    __syncthreads();
    if (threadIdx.x < 3) partials[p * 3 + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// one workgroup: out5 = {sum AA, sum BB, sum AB, cnt_a, cnt_b}; thread t adds up rows t, t + 256, ... in that order, then a
// fixed tree over the 256 threads
__global__ __launch_bounds__(256) void k_mmd_final(int64_t a, int64_t b, const double* __restrict__ inv,
                                                   const double* __restrict__ partials, double* __restrict__ out5) {
    __shared__ double sh[5][256];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r = threadIdx.x; r < a + b; r += 256) {
        for (int c = 0; c < 3; ++c) v[c] += partials[r * 3 + c];
        if (inv[r] > 0.0) v[r < a ? 3 : 4] += 1.0;
    }
    for (int c = 0; c < 5; ++c) sh[c][threadIdx.x] = v[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int c = 0; c < 5; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 5) out5[threadIdx.x] = sh[threadIdx.x][0];
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_graph_stats_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_nodes < 0 || max_nodes_per_graph < 0) return 0;
    return stats_ws(n_nodes, max_nodes_per_graph).total;
}

int gnf_graph_stats(const GnfCsr* csr, int32_t max_nodes_per_graph, int32_t clustering_bins, int32_t* degree,
                    int32_t* triangles, int32_t* degree_hist, int32_t* clustering_hist, int64_t* n_edges,
                    int64_t* n_triangles, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_graph_stats";
    if (int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kStatsMaxNodes, "a node's triangle count must fit int32")) return rc;
    if (clustering_bins < 1) {
        set_error("%s: clustering_bins=%d (bins >= 1)", what, clustering_bins);
        return GNF_ESHAPE;
    }
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    if ((n > 0 && (!degree || !triangles || !ws)) ||
        (b > 0 && (!clustering_hist || !n_edges || !n_triangles || (max_nodes_per_graph > 0 && !degree_hist)))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const StatsWs L = stats_ws(n, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    if (b == 0) return GNF_OK;   // an empty batch: nothing to write
    hipStream_t st = (hipStream_t)stream;
    if (max_nodes_per_graph > 0)
        GNF_HIP_TRY(hipMemsetAsync(degree_hist, 0, (size_t)b * (size_t)max_nodes_per_graph * sizeof(int32_t), st));
    GNF_HIP_TRY(hipMemsetAsync(clustering_hist, 0, (size_t)b * (size_t)clustering_bins * sizeof(int32_t), st));
    GNF_HIP_TRY(hipMemsetAsync(n_edges, 0, (size_t)b * sizeof(int64_t), st));
    GNF_HIP_TRY(hipMemsetAsync(n_triangles, 0, (size_t)b * sizeof(int64_t), st));
    if (n == 0) return GNF_OK;
    unsigned long long* bitmap = (unsigned long long*)((char*)ws + L.bitmap);
    int32_t* gid = (int32_t*)((char*)ws + L.gid);
    if (int rc = build_graph_bitmap(csr, max_nodes_per_graph, L.W, bitmap, gid, st)) return rc;
    const size_t lds = (size_t)L.W * sizeof(uint64_t) + 128 * sizeof(int32_t);   // <= 8.5 KB
    hipLaunchKernelGGL(k_stats_nodes, dim3(stats_grid(n)), dim3(64), lds, st, csr->node_offsets, n, max_nodes_per_graph, L.W,
                       clustering_bins, bitmap, gid, degree, triangles, degree_hist, clustering_hist,
                       (unsigned long long*)n_edges, (unsigned long long*)n_triangles);
    GNF_LAUNCH_CHECK("k_stats_nodes");
    hipLaunchKernelGGL(k_stats_finish, dim3(stats_grid((b + 255) / 256)), dim3(256), 0, st, b, n_edges, n_triangles);
    GNF_LAUNCH_CHECK("k_stats_finish");
    return GNF_OK;
}

size_t gnf_hist_mmd_workspace_bytes(int64_t a, int64_t b) {
    if (a < 0 || b < 0) return 0;
    return (size_t)(a + b) * 4 * sizeof(double);
}

int gnf_hist_mmd_f64(const int32_t* ha, int64_t a, int64_t lda, int32_t La, const int32_t* hb, int64_t b, int64_t ldb,
                     int32_t Lb, int32_t kernel, double sigma, double distance_scaling, double* out5, void* ws,
                     size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_hist_mmd_f64";
    if (a < 0 || b < 0 || La < 0 || Lb < 0 || La > lda || Lb > ldb || a + b > 0x7fffffff) {
        set_error("%s: a=%lld lda=%lld La=%d b=%lld ldb=%lld Lb=%d", what, (long long)a, (long long)lda, La, (long long)b,
                  (long long)ldb, Lb);
        return GNF_ESHAPE;
    }
    if (kernel != GNF_MMD_GAUSSIAN_EMD && kernel != GNF_MMD_GAUSSIAN_TV) {
        set_error("%s: kernel=%d", what, kernel);
        return GNF_EINVAL;
    }
    if (!(sigma > 0.0) || !(distance_scaling > 0.0)) {
        set_error("%s: sigma=%g distance_scaling=%g must be positive", what, sigma, distance_scaling);
        return GNF_EINVAL;
    }
    if (!out5 || (a > 0 && La > 0 && !ha) || (b > 0 && Lb > 0 && !hb) || (a + b > 0 && !ws)) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const size_t need = gnf_hist_mmd_workspace_bytes(a, b);
    if (ws_bytes < need) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, need);
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = a + b;
    if (n == 0) {   // two empty sets: five zeros
        GNF_HIP_TRY(hipMemsetAsync(out5, 0, 5 * sizeof(double), st));
        return GNF_OK;
    }
    const MmdSets s = {ha, hb, a, b, lda, ldb, La, Lb};
    double* inv = (double*)ws;
    double* partials = inv + n;
    hipLaunchKernelGGL(k_mmd_rowsums, dim3(stats_grid((n + 3) / 4)), dim3(256), 0, st, s, inv);
    GNF_LAUNCH_CHECK("k_mmd_rowsums");
    hipLaunchKernelGGL(k_mmd_pairs, dim3((unsigned)n), dim3(256), 0, st, s, kernel == GNF_MMD_GAUSSIAN_EMD ? 1 : 0,
                       1.0 / distance_scaling, -0.5 / (sigma * sigma), inv, partials);
    GNF_LAUNCH_CHECK("k_mmd_pairs");
    hipLaunchKernelGGL(k_mmd_final, dim3(1), dim3(256), 0, st, a, b, inv, partials, out5);
    GNF_LAUNCH_CHECK("k_mmd_final");
    return GNF_OK;
}

}  // extern "C"
