// Adjacency reconstruction loss of embeddings against a true batch (include/gnf_adj_loss.h): binary_loss
// (loss.py:162-188 of the reference), the edge-error counts (loss.py:88-116) and dL/dnodes, without the dense [N, N] true_adj /
// pred_adj / ce_loss matrices the reference builds and differentiates through.
//
// True graph.  Two DIRECTED bitmaps in the layout of gnf_graph_stats.hip (one 64-bit word per (node, 64 graph-local columns)),
// zeroed by k_adj_loss_zero, then filled from the receiver-sorted CSR by one wave per row with 64-bit integer atomicOr: for an
// entry (receiver i, sender j), i != j, both inside the graph's window,
//   in [i]  bit (j - n0): a_ji - "senders into row i"        out[j]  bit (i - n0): a_ji - "receivers out of row j"
// so a lane that works on the pair (i, j) finds a_ij in row i of `out` and a_ji in row i of `in`: both words of its own row.
//
// Pairs.  One workgroup per (graph, 16-row tile) walks the graph's columns in chunks of CJ (64, or 32 when that is what LDS
// holds).  Pass A: a lane owns one column of the chunk and CJ / 16 rows of the tile; d2 is pair_d2's fmaf chain and u the
// spelled-out logit k_pred_adj uses, p is written as there (same bits), then the two counts, the cross-entropy term (its three terms added in
// fp64) and c_ij, which goes to LDS.  Pass B: lanes over (row, feature) add c_ij (z_i - z_j) over the chunk's columns into
// the row's gradient, which the workgroup owns (written after the first chunk, plain read-modify-write after the others; no
// atomics).  A column with c_ij = 0 - a clipped pair, the diagonal - is skipped, not multiplied: it adds exactly nothing, as in
// the reference, even where an embedding is not finite.  Rows that no graph covers are zeroed by the bitmap kernel.
// z_i (the tile) and z_j (the chunk) sit in LDS while 64 KB hold them; wider rows keep the tile only, then nothing
// (same arithmetic in the same order, operands read from global memory).
// Row sums (fp64 loss, int32 counts) leave through a fixed shuffle tree and go to the workspace; one wave per graph adds
// its rows up, one wave the graphs: no floating-point atomics anywhere, two calls give the same bits.
//
// gnf_adj_loss_f32 and gnf_adj_loss_dist_f32 (include/gnf_distance.h) are one path: temp and shift may come from device memory
// (every workgroup loads them once and derives coef), the logit is gnf_distance_dev.h's spelled-out form, and two more fp64 row
// sums - (p - t) w and p - t over the pairs the clip leaves alone - ride the same shuffle tree; with grad_params they are
// stored, the two reducing kernels add them up in the loss's order and dL/dtemp, dL/dshift are rounded to fp32 once.
#include "gnf_distance_dev.h"
#include "gnf_graph_bitmap.h"

namespace gnf {

static constexpr int kAdjLossMaxNodes = 65536;   // a row's pair count fits int32; the grid's y extent stays below 65536
static constexpr int kAdjTile = 16;
static constexpr size_t kAdjLdsMax = 64 * 1024;
// U = log((1 - 1e-7) / 1e-7): Keras' epsilon clip of the probability, seen from the logit
static constexpr float kAdjClipU = 16.118095550958316f;

// caller-owned workspace (host only): in uint64 [N][W] | out uint64 [N][W] | row loss double [N] | row fp int32 [N] | row fn int32 [N]
// - `total` bytes, all gnf_adj_loss_f32 is given - then gnf_adj_loss_dist_f32's tail, `dist_total` in all, touched with
// grad_params only: row dtemp double [N] | row dshift double [N] | graph dtemp double [B] | graph dshift double [B]
struct AdjLossWs {
    size_t in, out, row_loss, row_fp, row_fn, total;
    size_t row_dtemp, row_dshift, graph_dtemp, graph_dshift, dist_total;
    int64_t W;
};
inline AdjLossWs adj_loss_ws(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes) {
    AdjLossWs L;
    L.W = ((int64_t)max_nodes + 63) / 64;
    const size_t bm = (size_t)n_nodes * (size_t)L.W * sizeof(uint64_t);
    L.in = 0;
    L.out = bm;
    L.row_loss = 2 * bm;
    L.row_fp = L.row_loss + (size_t)n_nodes * sizeof(double);
    L.row_fn = L.row_fp + (size_t)n_nodes * sizeof(int32_t);
    L.total = (L.row_fn + (size_t)n_nodes * sizeof(int32_t) + 7) / 8 * 8;
    L.row_dtemp = L.total;
    L.row_dshift = L.row_dtemp + (size_t)n_nodes * sizeof(double);
    L.graph_dtemp = L.row_dshift + (size_t)n_nodes * sizeof(double);
    L.graph_dshift = L.graph_dtemp + (size_t)n_graphs * sizeof(double);
    L.dist_total = L.graph_dshift + (size_t)n_graphs * sizeof(double);
    return L;
}

// one wave per CSR row i (receiver i): lanes take its entries 64 at a time.  An entry whose endpoints are not both inside the
// graph's [n0, n0 + ng) window is dropped (never an access outside the bitmaps).  grad != NULL: rows outside every graph's
// window get grad[i, 0:D) = 0 here (the pair kernel writes all the others).
__global__ __launch_bounds__(256) void k_adj_loss_bitmap(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         int64_t n_nodes, int64_t n_edges, const int32_t* __restrict__ off,
                                                         int64_t n_graphs, int max_nodes, int64_t W,
                                                         unsigned long long* __restrict__ in_bits,
                                                         unsigned long long* __restrict__ out_bits,
                                                         float* __restrict__ grad, int64_t ldg, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_nodes; i += (int64_t)gridDim.x * 4) {
        const int g = stats_graph_of(off, n_graphs, i);
        int64_t n0 = 0;
        int ng = 0;
        if (g >= 0) stats_graph_range(off, g, n_nodes, max_nodes, n0, ng);
        const int64_t li = i - n0;
        if (g < 0 || li < 0 || li >= ng) {   // a row no tile of the pair kernel covers: its gradient is zero
            if (grad)
                for (int f = lane; f < D; f += 64) grad[i * ldg + f] = 0.f;
            continue;
        }
        int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > n_edges) e1 = n_edges;
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int64_t lj = (int64_t)col[e] - n0;
            if (lj < 0 || lj >= ng || lj == li) continue;
            atomicOr(&in_bits[i * W + (lj >> 6)], 1ull << (lj & 63));
            atomicOr(&out_bits[(n0 + lj) * W + (li >> 6)], 1ull << (li & 63));
        }
    }
}

struct AdjLossParams {
    float temp, shift, scale;   // u = temp * (shift - d2 * scale)
    float t1, t0;               // label of a true edge / of a non-edge
    float abs_tol;
    float coef;                 // -2 temp scale
    float grad_scale;
    const float* params;        // NULL, or device {temp, shift}: temp, shift and coef are then re-read from it
    double* row_dtemp;          // NULL (no grad_params), or [n_nodes]: sum_j (p_ij - t_ij) w_ij, |u_ij| < U
    double* row_dshift;         // ... sum_j (p_ij - t_ij)
};

// LDS: cs [kAdjTile][CJ] | zi [kAdjTile][D] (ZI_LDS) | zj [CJ][Dp], Dp = D | 1 (ZJ_LDS: an odd row stride, lanes = columns)
template <int CJ, bool ZI_LDS, bool ZJ_LDS>
__global__ __launch_bounds__(256) void k_adj_loss_pairs(const float* __restrict__ z, int64_t ld, int D,
                                                        const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes,
                                                        int max_nodes, int64_t W,
                                                        const unsigned long long* __restrict__ in_bits,
                                                        const unsigned long long* __restrict__ out_bits, AdjLossParams P,
                                                        double* __restrict__ row_loss, int32_t* __restrict__ row_fp,
                                                        int32_t* __restrict__ row_fn, float* __restrict__ grad, int64_t ldg) {
    constexpr int RPT = CJ / kAdjTile;   // rows of the tile per lane
    constexpr int RSTEP = 256 / CJ;      // ... RSTEP apart
    extern __shared__ float adj_lds[];
    float* cs = adj_lds;
    float* zi = cs + kAdjTile * CJ;
    float* zj = zi + (ZI_LDS ? kAdjTile * D : 0);
    const int Dp = D | 1;
    const int i0 = blockIdx.y * kAdjTile;
    if (P.params) {   // (uniform: device-resident parameters, once per workgroup)
        P.temp = load_dist_param(P.params);
        P.shift = load_dist_param(P.params + 1);
        P.coef = __fmul_rn(-2.f * P.temp, P.scale);
    }
    for (int64_t g = blockIdx.x; g < n_graphs; g += gridDim.x) {   // (everything up to the lane's own pairs is uniform)
        int64_t n0;
        int ng;
        stats_graph_range(off, (int)g, n_nodes, max_nodes, n0, ng);
        if (i0 >= ng) continue;
        const int rows = ng - i0 < kAdjTile ? ng - i0 : kAdjTile;
        const int t = threadIdx.x;
        const int c = t & (CJ - 1), r0 = t / CJ;
        __syncthreads();   // the previous graph's readers of zi are done
        if constexpr (ZI_LDS) stage_row_tile(zi, z, ld, D, n0 + i0, rows);
        double ls[RPT];
        double dts[RPT], dss[RPT];   // the parameter gradient's row sums
        int fpc[RPT], fnc[RPT];
        const float* zr[RPT];
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            ls[k] = 0.0;
            dts[k] = dss[k] = 0.0;
            fpc[k] = fnc[k] = 0;
            int r = r0 + k * RSTEP;
            if (r >= rows) r = rows - 1;   // a row past the tile's end reads the last one; its results are dropped
            zr[k] = ZI_LDS ? zi + r * D : z + (n0 + i0 + r) * ld;
        }
        for (int j0 = 0; j0 < ng; j0 += CJ) {
            const int cn = ng - j0 < CJ ? ng - j0 : CJ;
            __syncthreads();   // the previous chunk's pass B is done with cs and zj
            if constexpr (ZJ_LDS) {
                for (int idx = t; idx < cn * D; idx += 256) {
                    const int cl = idx / D, f = idx - cl * D;
                    zj[cl * Dp + f] = z[(n0 + j0 + cl) * ld + f];
                }
                __syncthreads();
            }
            // ---- pass A: lane = (column c, rows r0 + k RSTEP)
            float cij[RPT];
#pragma unroll
            for (int k = 0; k < RPT; ++k) cij[k] = 0.f;
            if (c < cn) {
                const int j = j0 + c;
                const float* zc = ZJ_LDS ? zj + c * Dp : z + (n0 + j) * ld;
                float d2[RPT];
                pair_d2(zr, zc, D, d2);
                const int64_t w = j >> 6;
                const int bit = j & 63;
#pragma unroll
                for (int k = 0; k < RPT; ++k) {
                    const int r = r0 + k * RSTEP;
                    const int i = i0 + r;
                    if (r >= rows || i == j) continue;
                    const float wij = fmaf(-d2[k], P.scale, P.shift);   // w_ij = shift - d2 scale
                    const float u = __fmul_rn(P.temp, wij);             // sigmoid_l2_logit, with w_ij kept
                    const float p = 1.f / (1.f + expf(-u));
                    const int64_t word = (n0 + i) * W + w;
                    const bool aij = (out_bits[word] >> bit) & 1ull, aji = (in_bits[word] >> bit) & 1ull;
                    const float af = aij ? 1.f : 0.f;
                    if (p - af > P.abs_tol) ++fpc[k];
                    if (af - p > P.abs_tol) ++fnc[k];
                    const float tij = aij ? P.t1 : P.t0, tji = aji ? P.t1 : P.t0;
                    const float uc = fminf(fmaxf(u, -kAdjClipU), kAdjClipU);
                    ls[k] += ((double)fmaxf(uc, 0.f) + (double)log1pf(expf(-fabsf(uc)))) - (double)tij * (double)uc;
                    if (fabsf(u) < kAdjClipU) {
                        cij[k] = P.coef * ((p - tij) + (p - tji));
                        const double e = (double)(p - tij);
                        dts[k] += e * (double)wij;
                        dss[k] += e;
                    }
                }
            }
            if (grad) {   // (uniform)
#pragma unroll
                for (int k = 0; k < RPT; ++k) cs[(r0 + k * RSTEP) * CJ + c] = cij[k];
                __syncthreads();
                // ---- pass B: lane = (row, feature); the difference form, column by column in ascending order
                const bool last = j0 + CJ >= ng;
                for (int idx = t; idx < rows * D; idx += 256) {
                    const int rl = idx / D, f = idx - rl * D;
                    const float zif = ZI_LDS ? zi[idx] : z[(n0 + i0 + rl) * ld + f];
                    float* gp = grad + (n0 + i0 + rl) * ldg + f;
                    float acc = j0 == 0 ? 0.f : *gp;
                    const float* crow = cs + rl * CJ;
                    for (int cl = 0; cl < cn; ++cl) {
                        const float cv = crow[cl];
                        if (cv == 0.f) continue;   // clipped pair / diagonal: exactly nothing
                        const float zjf = ZJ_LDS ? zj[cl * Dp + f] : z[(n0 + j0 + cl) * ld + f];
                        acc = fmaf(cv, zif - zjf, acc);
                    }
                    *gp = last ? acc * P.grad_scale : acc;
                }
            }
        }
        // ---- row sums: the CJ lanes of a row, a fixed tree
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            double l = ls[k];
            int a = fpc[k], b = fnc[k];
            for (int o = CJ / 2; o > 0; o >>= 1) {
                l += __shfl_down(l, o, CJ);
                a += __shfl_down(a, o, CJ);
                b += __shfl_down(b, o, CJ);
            }
            const int r = r0 + k * RSTEP;
            if (c == 0 && r < rows) {
                row_loss[n0 + i0 + r] = l;
                row_fp[n0 + i0 + r] = a;
                row_fn[n0 + i0 + r] = b;
            }
            double dt = dts[k], ds = dss[k];
            for (int o = CJ / 2; o > 0; o >>= 1) {
                dt += __shfl_down(dt, o, CJ);
                ds += __shfl_down(ds, o, CJ);
            }
            if (c == 0 && r < rows && P.row_dtemp) {
                P.row_dtemp[n0 + i0 + r] = dt;
                P.row_dshift[n0 + i0 + r] = ds;
            }
        }
    }
}

// one wave per graph: lane l adds rows l, l + 64, ... in that order, then the wave's fixed tree.  row_dtemp != NULL (grad_params;
// uniform): the two row sums of the parameter gradient go the same way into graph_dtemp / graph_dshift.
__global__ __launch_bounds__(256) void k_adj_loss_graphs(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes,
                                                         int max_nodes, const double* __restrict__ row_loss,
                                                         const int32_t* __restrict__ row_fp, const int32_t* __restrict__ row_fn,
                                                         const double* __restrict__ row_dtemp,
                                                         const double* __restrict__ row_dshift,
                                                         double* __restrict__ loss_per_graph, int64_t* __restrict__ fp_pairs,
                                                         int64_t* __restrict__ fn_pairs, double* __restrict__ graph_dtemp,
                                                         double* __restrict__ graph_dshift) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool gp = row_dtemp != nullptr;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < n_graphs; g += (int64_t)gridDim.x * 4) {
        int64_t n0;
        int ng;
        stats_graph_range(off, (int)g, n_nodes, max_nodes, n0, ng);
        double l = 0.0, dt = 0.0, ds = 0.0;
        unsigned long long a = 0, b = 0;
        for (int r = lane; r < ng; r += 64) {
            l += row_loss[n0 + r];
            a += (unsigned long long)row_fp[n0 + r];
            b += (unsigned long long)row_fn[n0 + r];
            if (gp) {
                dt += row_dtemp[n0 + r];
                ds += row_dshift[n0 + r];
            }
        }
        l = wave_sum_f64(l);
        a = wave_sum_u64(a);
        b = wave_sum_u64(b);
        if (gp) {
            dt = wave_sum_f64(dt);
            ds = wave_sum_f64(ds);
        }
        if (lane == 0) {
            loss_per_graph[g] = l;
            fp_pairs[g] = (int64_t)a;
            fn_pairs[g] = (int64_t)b;
            if (gp) {
                graph_dtemp[g] = dt;
                graph_dshift[g] = ds;
            }
        }
    }
}

// one wave: sums2 = { sum_g loss_per_graph[g], that / (N^2 - N) } and, with grad_params (uniform),
// grad_params = grad_scale * { sum_g dtemp[g], temp * sum_g dshift[g] } rounded to fp32 once
__global__ __launch_bounds__(64) void k_adj_loss_total(int64_t n_graphs, int64_t n_nodes,
                                                       const double* __restrict__ loss_per_graph,
                                                       const double* __restrict__ graph_dtemp,
                                                       const double* __restrict__ graph_dshift, float temp,
                                                       const float* __restrict__ params, float grad_scale,
                                                       double* __restrict__ sums2, float* __restrict__ grad_params) {
    double l = 0.0, dt = 0.0, ds = 0.0;
    for (int64_t g = threadIdx.x; g < n_graphs; g += 64) {
        l += loss_per_graph[g];
        if (grad_params) {
            dt += graph_dtemp[g];
            ds += graph_dshift[g];
        }
    }
    l = wave_sum_f64(l);
    if (grad_params) {
        dt = wave_sum_f64(dt);
        ds = wave_sum_f64(ds);
    }
    if (threadIdx.x == 0) {
        sums2[0] = l;
        sums2[1] = n_nodes < 2 ? 0.0 : l / ((double)n_nodes * (double)n_nodes - (double)n_nodes);
        if (grad_params) {
            if (params) temp = load_dist_param(params);
            grad_params[0] = (float)((double)grad_scale * dt);
            grad_params[1] = (float)((double)grad_scale * ((double)temp * ds));
        }
    }
}

// The workspace is zeroed by a kernel, not a memset: in a captured graph that is replayed, a memset node is not reliably
// finished before the kernel nodes behind it start (bits of the bitmaps and whole row sums went missing from the second replay
// on), and both entry points are captured by the trainer
__global__ __launch_bounds__(256) void k_adj_loss_zero(unsigned long long* __restrict__ ws, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) ws[i] = 0ull;
}

// the two entry points.  dist == NULL: gnf_adj_loss_f32 - spec's distance, and a workspace without the parameter gradient's tail
static int adj_loss(const char* what, const GnfCsr* csr, const float* z, int64_t ld, int32_t D, int32_t max_nodes_per_graph,
                    const GnfAdjLossSpec* spec, const GnfDistance* dist, double* loss_per_graph, double* sums2,
                    int64_t* fp_pairs, int64_t* fn_pairs, float* grad, int64_t ld_grad, float grad_scale, float* grad_params,
                    void* ws, size_t ws_bytes, gnf_stream_t stream) {
    if (int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kAdjLossMaxNodes, "a row's pair count fits int32")) return rc;
    if (!spec) {
        set_error("%s: null spec", what);
        return GNF_EINVAL;
    }
    if (D < 1 || ld < D || (grad && ld_grad < D)) {
        set_error("%s: D=%d ld=%lld ld_grad=%lld", what, D, (long long)ld, (long long)ld_grad);
        return GNF_ESHAPE;
    }
    if (!(spec->label_epsilon >= 0.f && spec->label_epsilon <= 0.5f) || !(spec->abs_tol >= 0.f)) {
        set_error("%s: label_epsilon=%g (in [0, 0.5]) abs_tol=%g (>= 0)", what, (double)spec->label_epsilon,
                  (double)spec->abs_tol);
        return GNF_ESHAPE;
    }
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    if (!sums2 || (n > 0 && (!z || !ws)) || (b > 0 && (!loss_per_graph || !fp_pairs || !fn_pairs))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const AdjLossWs L = adj_loss_ws(b, n, max_nodes_per_graph);
    const size_t need = dist ? L.dist_total : L.total;
    if (ws_bytes < need) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, need);
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || b == 0) {   // nothing to score: zeros
        GNF_HIP_TRY(hipMemsetAsync(sums2, 0, 2 * sizeof(double), st));
        if (grad_params) GNF_HIP_TRY(hipMemsetAsync(grad_params, 0, 2 * sizeof(float), st));
        if (b > 0) {
            GNF_HIP_TRY(hipMemsetAsync(loss_per_graph, 0, (size_t)b * sizeof(double), st));
            GNF_HIP_TRY(hipMemsetAsync(fp_pairs, 0, (size_t)b * sizeof(int64_t), st));
            GNF_HIP_TRY(hipMemsetAsync(fn_pairs, 0, (size_t)b * sizeof(int64_t), st));
        }
        return GNF_OK;
    }
    unsigned long long* in_bits = (unsigned long long*)((char*)ws + L.in);
    unsigned long long* out_bits = (unsigned long long*)((char*)ws + L.out);
    double* row_loss = (double*)((char*)ws + L.row_loss);
    int32_t* row_fp = (int32_t*)((char*)ws + L.row_fp);
    int32_t* row_fn = (int32_t*)((char*)ws + L.row_fn);
    // bitmaps, and the sums of rows no tile covers - the parameter gradient's among them, in the tail that only a call with
    // grad_params owns (every offset of the layout is a multiple of 8, and so is ws: it starts with the uint64 bitmaps)
    const size_t words = (grad_params ? L.graph_dtemp : L.total) / sizeof(unsigned long long);
    hipLaunchKernelGGL(k_adj_loss_zero, dim3(stats_grid((int64_t)((words + 255) / 256))), dim3(256), 0, st,
                       (unsigned long long*)ws, words);
    GNF_LAUNCH_CHECK("k_adj_loss_zero");
    hipLaunchKernelGGL(k_adj_loss_bitmap, dim3(stats_grid((n + 3) / 4)), dim3(256), 0, st, csr->rowptr, csr->col, n,
                       csr->n_edges, csr->node_offsets, b, max_nodes_per_graph, L.W, in_bits, out_bits, grad, ld_grad, D);
    GNF_LAUNCH_CHECK("k_adj_loss_bitmap");
    const DistSigmoid ds = dist ? dist_sigmoid(*dist, D)
                                : dist_sigmoid(spec->temp, spec->shift, spec->scale_by_sqrt_dim, nullptr, D);
    AdjLossParams P;
    P.temp = ds.temp;
    P.shift = ds.shift;
    P.scale = ds.scale;
    P.t1 = spec->soft_labels ? 1.f - spec->label_epsilon : 1.f;
    P.t0 = spec->soft_labels ? spec->label_epsilon : 0.f;
    P.abs_tol = spec->abs_tol;
    P.coef = -2.f * P.temp * P.scale;
    P.grad_scale = grad_scale;
    P.params = ds.params;
    P.row_dtemp = grad_params ? (double*)((char*)ws + L.row_dtemp) : nullptr;
    P.row_dshift = grad_params ? (double*)((char*)ws + L.row_dshift) : nullptr;
    double* graph_dtemp = grad_params ? (double*)((char*)ws + L.graph_dtemp) : nullptr;
    double* graph_dshift = grad_params ? (double*)((char*)ws + L.graph_dshift) : nullptr;
    const dim3 grid(stats_grid(b), (unsigned)((max_nodes_per_graph + kAdjTile - 1) / kAdjTile));
    const size_t tile = (size_t)kAdjTile * D * sizeof(float), dp = (size_t)(D | 1) * sizeof(float);
    const size_t cs64 = (size_t)kAdjTile * 64 * sizeof(float), cs32 = (size_t)kAdjTile * 32 * sizeof(float);
#define GNF_ADJ_LAUNCH(CJ, ZI, ZJ, LDS)                                                                                       \
    hipLaunchKernelGGL((k_adj_loss_pairs<CJ, ZI, ZJ>), grid, dim3(256), LDS, st, z, ld, D, csr->node_offsets, b, n,          \
                       max_nodes_per_graph, L.W, in_bits, out_bits, P, row_loss, row_fp, row_fn, grad, ld_grad)
    if (cs64 + tile + 64 * dp <= kAdjLdsMax)
        GNF_ADJ_LAUNCH(64, true, true, cs64 + tile + 64 * dp);
    else if (cs32 + tile + 32 * dp <= kAdjLdsMax)
        GNF_ADJ_LAUNCH(32, true, true, cs32 + tile + 32 * dp);
    else if (cs64 + tile <= kAdjLdsMax)
        GNF_ADJ_LAUNCH(64, true, false, cs64 + tile);
    else
        GNF_ADJ_LAUNCH(64, false, false, cs64);
#undef GNF_ADJ_LAUNCH
    GNF_LAUNCH_CHECK("k_adj_loss_pairs");
    hipLaunchKernelGGL(k_adj_loss_graphs, dim3(stats_grid((b + 3) / 4)), dim3(256), 0, st, csr->node_offsets, b, n,
                       max_nodes_per_graph, row_loss, row_fp, row_fn, P.row_dtemp, P.row_dshift, loss_per_graph, fp_pairs,
                       fn_pairs, graph_dtemp, graph_dshift);
    GNF_LAUNCH_CHECK("k_adj_loss_graphs");
    hipLaunchKernelGGL(k_adj_loss_total, dim3(1), dim3(64), 0, st, b, n, loss_per_graph, graph_dtemp, graph_dshift, P.temp,
                       P.params, grad_scale, sums2, grad_params);
    GNF_LAUNCH_CHECK("k_adj_loss_total");
    return GNF_OK;
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_adj_loss_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_nodes < 0 || max_nodes_per_graph < 0) return 0;
    return adj_loss_ws(n_graphs, n_nodes, max_nodes_per_graph).total;
}

int gnf_adj_loss_f32(const GnfCsr* csr, const float* z, int64_t ld, int32_t D, int32_t max_nodes_per_graph,
                     const GnfAdjLossSpec* spec, double* loss_per_graph, double* sums2, int64_t* fp_pairs, int64_t* fn_pairs,
                     float* grad, int64_t ld_grad, float grad_scale, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    return adj_loss("gnf_adj_loss_f32", csr, z, ld, D, max_nodes_per_graph, spec, nullptr, loss_per_graph, sums2, fp_pairs,
                    fn_pairs, grad, ld_grad, grad_scale, nullptr, ws, ws_bytes, stream);
}

size_t gnf_adj_loss_dist_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_nodes < 0 || max_nodes_per_graph < 0) return 0;
    return adj_loss_ws(n_graphs, n_nodes, max_nodes_per_graph).dist_total;
}

int gnf_adj_loss_dist_f32(const GnfCsr* csr, const float* z, int64_t ld, int32_t D, int32_t max_nodes_per_graph,
                          const GnfAdjLossSpec* spec, const GnfDistance* dist, double* loss_per_graph, double* sums2,
                          int64_t* fp_pairs, int64_t* fn_pairs, float* grad, int64_t ld_grad, float grad_scale,
                          float* grad_params, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    if (!dist) {
        set_error("gnf_adj_loss_dist_f32: null dist");
        return GNF_EINVAL;
    }
    return adj_loss("gnf_adj_loss_dist_f32", csr, z, ld, D, max_nodes_per_graph, spec, dist, loss_per_graph, sums2, fp_pairs,
                    fn_pairs, grad, ld_grad, grad_scale, grad_params, ws, ws_bytes, stream);
}

}  // extern "C"
