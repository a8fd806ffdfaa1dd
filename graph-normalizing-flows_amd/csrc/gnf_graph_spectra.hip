// Scoring generated graphs on the device, fourth statistic: the eigenvalues of every graph's normalised Laplacian and their
// per-graph histogram - next to the degree / clustering MMD of gnf_graph_stats.hip and the orbit MMD of gnf_graph_orbits.hip the
// number graph-generation papers since GRAN report (the MMD itself is gnf_hist_mmd_f64 on the histograms).  The reference
// stops at pickling the graphs (generate_graphs.py:68-84); nothing in it corresponds to this kernel.
//
// Graph model and bitmap: as in gnf_graph_stats.hip (undirected, simple), built by build_graph_bitmap (gnf_graph_bitmap.h:
// k_stats_bitmap on a zeroed bitmap).  L_ii = 1 if d_i > 0 else 0, L_ij = -1 / sqrt(d_i d_j) for an edge, else 0.
//
// Launches: k_stats_bitmap; k_spectra<LDS, NT> - one workgroup of NT threads per graph slot, everything in fp64:
//   1. degrees by popcount of the bitmap rows; L formed densely (both triangles) in the slot's matrix S [n_g][n_g].
//   2. Householder tridiagonalisation.  Column k = 0 .. n_g - 3, with x = S[k][k+1 ..] (row k, by symmetry column k):
//        sigma2 = |x|^2;  sigma2 == 0: e_k = 0, nothing to do.  Else alpha = -sign(x_0) |x|, v = x - alpha e_0,
//        beta = 2 / v'v = 1 / (sigma2 - alpha x_0),  p = beta S v  (thread i: sum_j S[j][i] v_j - rows of S read across the
//        threads, so LDS banks / global lines are hit side by side),  K = beta/2 v'p,  w = p - K v,  S -= v w' + w v'  on the
//        trailing block (a wave per row).  d_k = S[k][k], e_k = alpha.  No scaling of x: |S_ij| <= |L|_2 <= 2 throughout.
//      The two sums per column (|x|^2, v'p) are a fixed tree: per thread in index order, 64 lanes by shuffles, the waves in order.
//   3. Bisection on Sturm counts of the tridiagonal (d, e^2): thread j finds eigenvalue j from the interval [-0.5, 2.5]
//      (Gershgorin: the spectrum lies in [0, 2]) with exactly 64 halvings - no convergence test; a pivot below kPivMin in
//      magnitude is replaced by -kPivMin (LAPACK dlaebz's rule), so nothing divides by zero.  The values come out ascending.
//   4. Histogram: kHistChunk bins at a time in LDS with integer atomics, each chunk then stored - the whole row is written.
// Every loop is bounded by n_g, max_nodes_per_graph, bins or a constant; the result does not depend on the order in which
// anything runs, so two calls give the same bits.  Error: Householder and bisection are backward stable, |error| <= c n u |L|_2.
//
// Routes, per call from max_nodes_per_graph (cap):
//   cap <= kSpectraLdsNodes   S in LDS: 8 cap^2 + 32 cap + 4224 bytes (<= 160 KiB at 139), one workgroup of 256 threads per graph
//   else                      S in the workspace: min(n_graphs, kSpectraSlots) slots of cap^2 doubles, workgroup w takes graphs
//                             w, w + kSpectraSlots, ... (the barrier that opens a graph orders the slot's reuse); 1024 threads:
//                             the rank-2 update and the product S v wait on memory, sixteen waves keep more of it in flight
#include "gnf_graph_bitmap.h"
#include "gnf_options.h"

namespace gnf {

static constexpr int kSpectraMaxNodes = GNF_SPECTRA_MAX_NODES;
static constexpr int kSpectraLdsNodes = GNF_SPECTRA_LDS_NODES;
static constexpr int kSpectraSlots = GNF_SPECTRA_SLOTS;
static constexpr int kSpectraBlockLds = 256, kSpectraBlockWs = 1024;   // threads per workgroup, by route
static constexpr int kHistChunk = 1024;
static constexpr int kBisectSteps = 64;
static constexpr double kPivMin = 1e-290;   // e^2 <= 4: e^2 / kPivMin stays finite
static constexpr size_t kSpectraLdsFixed = 128 + kHistChunk * sizeof(int32_t);   // wave partials [16] | histogram chunk
static_assert(8ull * kSpectraLdsNodes * kSpectraLdsNodes + 32ull * kSpectraLdsNodes + kSpectraLdsFixed <= 160 * 1024 &&
              8ull * (kSpectraLdsNodes + 1) * (kSpectraLdsNodes + 1) + 32ull * (kSpectraLdsNodes + 1) + kSpectraLdsFixed > 160 * 1024,
              "kSpectraLdsNodes is the largest graph whose matrix fits 160 KiB of LDS");
static_assert(32ull * kSpectraMaxNodes + kSpectraLdsFixed <= 160 * 1024, "the vectors of the workspace route fit LDS");

// caller-owned workspace of gnf_graph_spectra (host only): the gnf_graph_stats workspace (bitmap, gid) | slots double [slots][cap^2]
struct SpectraWs {
    StatsWs stats;
    size_t mats, total;
    int64_t slots;
};
static SpectraWs spectra_ws(int64_t n_graphs, int64_t n_nodes, int32_t cap) {
    SpectraWs L;
    L.stats = stats_ws(n_nodes, cap);
    L.mats = L.stats.total;
    L.slots = cap > kSpectraLdsNodes ? (n_graphs < kSpectraSlots ? n_graphs : kSpectraSlots) : 0;
    L.total = L.mats + (size_t)L.slots * (size_t)cap * (size_t)cap * sizeof(double);
    return L;
}
static size_t spectra_lds_bytes(int32_t cap) {
    return (cap <= kSpectraLdsNodes ? 8 * (size_t)cap * cap : 0) + 32 * (size_t)cap + kSpectraLdsFixed;
}

// sum over the workgroup in a fixed order; every thread gets it.  part: NT / 64 doubles of LDS
template <int NT>
__device__ __forceinline__ double spectra_block_sum(double v, double* part, int tid) {
    v = wave_sum_f64(v);
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    double r = part[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r += part[w];
    __syncthreads();
    return r;
}

// LDS (doubles first): [S cap^2 if LDS_MAT] | dd [cap] | esq [cap] | v [cap] | p [cap] | part [16] | hist chunk int32 [kHistChunk]
template <bool LDS_MAT, int NT>
__global__ __launch_bounds__(NT) void k_spectra(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes, int cap,
                                                int64_t W, const unsigned long long* __restrict__ bitmap, double* mats,
                                                double* __restrict__ eig, int32_t* __restrict__ hist, int bins, double lo,
                                                double hi) {
    extern __shared__ double spectra_lds[];
    const size_t mat_elems = LDS_MAT ? (size_t)cap * cap : 0;
    double* dd = spectra_lds + mat_elems;
    double* esq = dd + cap;
    double* v = esq + cap;
    double* p = v + cap;
    double* part = p + cap;
    int32_t* hchunk = (int32_t*)(part + 16);
    int32_t* deg = (int32_t*)p;   // (during the formation of L only)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* S;
    if constexpr (LDS_MAT) S = spectra_lds;
    else S = mats + (size_t)blockIdx.x * (size_t)cap * (size_t)cap;

    for (int64_t g = blockIdx.x; g < n_graphs; g += gridDim.x) {   // (uniform over the workgroup)
        int64_t n0;
        int n;
        stats_graph_range(off, (int)g, n_nodes, cap, n0, n);
        __syncthreads();   // the previous graph's readers are done
        // 1. degrees, L
        for (int i = tid; i < n; i += NT) {
            const unsigned long long* row = bitmap + (n0 + i) * W;
            int d = 0;
            for (int w = 0; w < (n + 63) / 64; ++w) d += __popcll(row[w]);
            deg[i] = d;
        }
        __syncthreads();
        for (int i = wave; i < n; i += NT / 64) {
            const unsigned long long* row = bitmap + (n0 + i) * W;
            const long long di = deg[i];
            for (int j = lane; j < n; j += 64) {
                double x = 0.0;
                if (j == i) x = di > 0 ? 1.0 : 0.0;
                else if ((row[j >> 6] >> (j & 63)) & 1ull) x = -1.0 / sqrt((double)(di * (long long)deg[j]));
                S[(size_t)i * n + j] = x;
            }
        }
        __syncthreads();
        // 2. Householder tridiagonalisation
        for (int k = 0; k + 2 < n; ++k) {
            const double* rowk = S + (size_t)k * n;
            double s2 = 0.0;
            for (int j = k + 1 + tid; j < n; j += NT) {
                const double x = rowk[j];
                v[j] = x;
                s2 += x * x;
            }
            const double sigma2 = spectra_block_sum<NT>(s2, part, tid);
            if (sigma2 == 0.0) {   // (uniform) the column is already reduced
                if (tid == 0) {
                    dd[k] = rowk[k];
                    esq[k] = 0.0;
                }
                continue;
            }
            const double x0 = v[k + 1];
            const double alpha = x0 >= 0.0 ? -sqrt(sigma2) : sqrt(sigma2);
            const double beta = 1.0 / (sigma2 - alpha * x0);
            __syncthreads();   // every thread has read x0
            if (tid == 0) {
                v[k + 1] = x0 - alpha;
                dd[k] = rowk[k];
                esq[k] = alpha * alpha;
            }
            __syncthreads();
            double vp = 0.0;
            for (int i = k + 1 + tid; i < n; i += NT) {
                const double* col = S + i;
                double s = 0.0;
#pragma unroll 8
                for (int j = k + 1; j < n; ++j) s += col[(size_t)j * n] * v[j];
                s *= beta;
                p[i] = s;
                vp += v[i] * s;
            }
            const double kc = 0.5 * beta * spectra_block_sum<NT>(vp, part, tid);
            for (int i = k + 1 + tid; i < n; i += NT) p[i] -= kc * v[i];   // w
            __syncthreads();
            for (int i = k + 1 + wave; i < n; i += NT / 64) {
                const double vi = v[i], wi = p[i];
                double* rowi = S + (size_t)i * n;
                for (int j = k + 1 + lane; j < n; j += 64) rowi[j] -= vi * p[j] + wi * v[j];
            }
            __syncthreads();
        }
        if (tid == 0 && n >= 1) {
            dd[n - 1] = S[(size_t)(n - 1) * n + (n - 1)];
            if (n >= 2) {
                const double e = S[(size_t)(n - 2) * n + (n - 1)];
                dd[n - 2] = S[(size_t)(n - 2) * n + (n - 2)];
                esq[n - 2] = e * e;
            }
        }
        __syncthreads();
        // 3. bisection: eigenvalue j = the point where the Sturm count (eigenvalues below x) passes j
        for (int j = tid; j < n; j += NT) {
            double a = -0.5, b = 2.5;
            for (int it = 0; it < kBisectSteps; ++it) {
                const double x = 0.5 * (a + b);
                double q = dd[0] - x;
                if (fabs(q) < kPivMin) q = -kPivMin;   // (before it is counted: x = 1, the first midpoint, meets d_0 = 1)
                int below = q < 0.0;
                for (int i = 1; i < n; ++i) {
                    q = dd[i] - x - esq[i - 1] / q;
                    if (fabs(q) < kPivMin) q = -kPivMin;
                    below += q < 0.0;
                }
                if (below > j) b = x; else a = x;
            }
            const double x = 0.5 * (a + b);
            eig[n0 + j] = x;
            v[j] = x;
        }
        __syncthreads();
        // 4. histogram, a chunk of bins at a time
        for (int64_t c0 = 0; c0 < bins; c0 += kHistChunk) {   // (64-bit: bins may be close to 2^31)
            const int cn = bins - c0 < kHistChunk ? (int)(bins - c0) : kHistChunk;
            for (int c = tid; c < cn; c += NT) hchunk[c] = 0;
            __syncthreads();
            for (int j = tid; j < n; j += NT) {
                double t = floor((v[j] - lo) * (double)bins / (hi - lo));
                t = t > 0.0 ? t : 0.0;   // (also a NaN)
                const int bin = t < (double)(bins - 1) ? (int)t : bins - 1;
                if (bin >= c0 && bin < c0 + cn) atomicAdd(&hchunk[bin - c0], 1);
            }
            __syncthreads();
            for (int c = tid; c < cn; c += NT) hist[g * bins + c0 + c] = hchunk[c];
            __syncthreads();
        }
    }
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_graph_spectra_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_nodes < 0 || max_nodes_per_graph < 0 || max_nodes_per_graph > kSpectraMaxNodes) return 0;
    return spectra_ws(n_graphs, n_nodes, max_nodes_per_graph).total;
}

int gnf_graph_spectra(const GnfCsr* csr, int32_t max_nodes_per_graph, double* eigenvalues, int32_t* hist, int32_t bins, double lo,
                      double hi, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_graph_spectra";
    if (int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kSpectraMaxNodes, "a dense eigenvalue solver, n^3 work per graph"))
        return rc;
    if (bins < 0 || (bins > 0 && !(hi > lo))) {
        set_error("%s: bins=%d lo=%g hi=%g (bins >= 0, and lo < hi with bins > 0)", what, bins, lo, hi);
        return GNF_ESHAPE;
    }
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    if (n > 0 && (!eigenvalues || !ws)) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    if (bins > 0 && b > 0 && !hist) {
        set_error("%s: hist is null with bins=%d", what, bins);
        return GNF_EINVAL;
    }
    const SpectraWs L = spectra_ws(b, n, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    if (b == 0) return GNF_OK;   // an empty batch: nothing to write
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {                // graphs without nodes: all-zero rows
        if (bins > 0) GNF_HIP_TRY(hipMemsetAsync(hist, 0, (size_t)b * (size_t)bins * sizeof(int32_t), st));
        return GNF_OK;
    }
    unsigned long long* bitmap = (unsigned long long*)((char*)ws + L.stats.bitmap);
    int32_t* gid = (int32_t*)((char*)ws + L.stats.gid);
    GNF_HIP_TRY(hipMemsetAsync(eigenvalues, 0, (size_t)n * sizeof(double), st));   // rows no graph (or no column) covers
    if (int rc = build_graph_bitmap(csr, max_nodes_per_graph, L.stats.W, bitmap, gid, st)) return rc;
    GNF_ONCE_PER_DEVICE(
        GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_spectra<true, kSpectraBlockLds>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_spectra<false, kSpectraBlockWs>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)));
    const size_t lds = spectra_lds_bytes(max_nodes_per_graph);
    if (L.slots == 0) {
        hipLaunchKernelGGL((k_spectra<true, kSpectraBlockLds>), dim3(stats_grid(b)), dim3(kSpectraBlockLds), lds, st,
                           csr->node_offsets, b, n, max_nodes_per_graph, L.stats.W, bitmap, (double*)nullptr, eigenvalues, hist,
                           bins, lo, hi);
        GNF_LAUNCH_CHECK("k_spectra<lds>");
    } else {
        hipLaunchKernelGGL((k_spectra<false, kSpectraBlockWs>), dim3((unsigned)L.slots), dim3(kSpectraBlockWs), lds, st,
                           csr->node_offsets, b, n, max_nodes_per_graph, L.stats.W, bitmap, (double*)((char*)ws + L.mats),
                           eigenvalues, hist, bins, lo, hi);
        GNF_LAUNCH_CHECK("k_spectra<workspace>");
    }
    return GNF_OK;
}

}  // extern "C"
