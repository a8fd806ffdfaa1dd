// The reconstruction report (include/gnf_adj_report.h): which ordered pairs of a batch embeddings get wrong against the true
// graph, as a classified edge list with scores, and exact order statistics of the scores of a class - what
// run_gnn_inference.py:107-163 of the reference works out on the host from dense [N, N] matrices.
//
// Count.  k_report_bitmap fills the "senders into row r" words from the receiver-sorted CSR as k_adj_loss_bitmap does (one wave
// per row, 64-bit integer atomicOr; only this orientation is needed) and copies the CSR's int32 node offsets into the int64
// ones the decoder's kernels and scan read.  k_report_count is k_edge_count's walk (gnf_decode_edges.hip: one workgroup per
// (graph, 16-row tile), wave w owns rows 4 w .. 4 w + 3, lane = column, one ballot per (row, 64 columns)) without self loops:
// the pred word goes to the workspace beside the true word, the row's entry count is popcount(pred | true) and its three
// class counts are popcounts too.  launch_edge_scan gives rowptr / n_edge / totals[0]; one wave per graph adds the rows' class
// counts up, one wave the graphs' - fixed order, integers.
// Fill.  k_edge_fill's expansion over pred | true; cls comes from the two words and the score is recomputed for the set bits
// only, through pair_d2 and DistSigmoid::logit and the sigmoid expression of k_pred_adj - the same bits.
// Select.  k_score_select: exact k-th smallest by radix selection on the scores' uint32 bit patterns, most significant byte
// first; one workgroup per (segment, class, q).
// No floating-point atomics, every word, count and entry has one writer (the OR atomics commute): two calls give the same bytes.
#include "gnf_distance_dev.h"
#include "gnf_edge_ws.h"
#include "gnf_graph_bitmap.h"

namespace gnf {

static constexpr int kReportMaxNodes = 65536;   // gnf_adj_loss_f32's bound: a row's pair count fits int32
static constexpr int kSelectThreads = 1024;

// caller-owned workspace of count and fill (host only):
// node_off int64 [B + 1] | true uint64 [N][W] | pred uint64 [N][W] | rowcnt int32 [N] | rowcls int32 [3][N]
struct ReportWs {
    size_t node_off, true_bits, pred_bits, rowcnt, rowcls, total;
    int64_t W;
};
inline ReportWs report_ws(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes) {
    ReportWs L;
    L.W = ((int64_t)max_nodes + 63) / 64;
    const size_t bm = (size_t)n_nodes * (size_t)L.W * sizeof(uint64_t);
    L.node_off = 0;
    L.true_bits = (size_t)(n_graphs + 1) * sizeof(int64_t);
    L.pred_bits = L.true_bits + bm;
    L.rowcnt = L.pred_bits + bm;
    L.rowcls = L.rowcnt + (size_t)n_nodes * sizeof(int32_t);
    L.total = (L.rowcls + 3 * (size_t)n_nodes * sizeof(int32_t) + 7) / 8 * 8;
    return L;
}

// zeroed by a kernel, not a memset: a memset node of a replayed capture is not reliably ordered before the kernels behind it
// (gnf_adj_loss.hip)
__global__ __launch_bounds__(256) void k_report_zero(uint32_t* __restrict__ p, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

// one wave per CSR row i (receiver i), lanes over its entries: bit (j - n0) of row i's words for every sender j != i inside the
// graph's window; anything else is dropped.  The first workgroup's lanes also copy the node offsets.
__global__ __launch_bounds__(256) void k_report_bitmap(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                       int64_t n_nodes, int64_t n_edges, const int32_t* __restrict__ off,
                                                       int64_t n_graphs, int max_nodes, int64_t W,
                                                       unsigned long long* __restrict__ true_bits,
                                                       int64_t* __restrict__ node_off) {
    if (blockIdx.x == 0)
        for (int64_t g = threadIdx.x; g <= n_graphs; g += 256) node_off[g] = off[g];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_nodes; i += (int64_t)gridDim.x * 4) {
        const int g = stats_graph_of(off, n_graphs, i);
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
            atomicOr(&true_bits[i * W + (lj >> 6)], 1ull << (lj & 63));
        }
    }
}

// rowcls: [0][i] class 1 (a & pred), [1][i] class 2 (!a & pred), [2][i] class 3 (a & !pred)
template <bool LDS_ROWS>
__global__ __launch_bounds__(256) void k_report_count(const float* __restrict__ z, int64_t ld, int D,
                                                      const int64_t* __restrict__ node_off, int64_t n_nodes, int max_nodes,
                                                      int64_t W, float threshold, DistSigmoid dist_arg,
                                                      const unsigned long long* __restrict__ true_bits,
                                                      unsigned long long* __restrict__ pred_bits, int32_t* __restrict__ rowcnt,
                                                      int32_t* __restrict__ rowcls) {
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
        int cnt[kEdgeWaveRows], c1[kEdgeWaveRows], c2[kEdgeWaveRows], c3[kEdgeWaveRows];
        for (int q = 0; q < kEdgeWaveRows; ++q) {
            const int rl = r0 + q < rows ? r0 + q : rows - 1;   // rows past the tile's end repeat its last row; not stored
            zr[q] = LDS_ROWS ? zi + rl * D : z + (n0 + i0 + rl) * ld;
            cnt[q] = c1[q] = c2[q] = c3[q] = 0;
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
                const unsigned long long pred = __ballot(col && i != j && p > threshold);
                if (r0 + q < rows) {
                    const unsigned long long tw = true_bits[(n0 + i) * W + w];   // (one address for the wave)
                    if (lane == 0) pred_bits[(n0 + i) * W + w] = pred;
                    cnt[q] += __popcll(pred | tw);
                    c1[q] += __popcll(pred & tw);
                    c2[q] += __popcll(pred & ~tw);
                    c3[q] += __popcll(tw & ~pred);
                }
            }
        }
        if (lane == 0)
            for (int q = 0; q < kEdgeWaveRows; ++q)
                if (r0 + q < rows) {
                    const int64_t row = n0 + i0 + r0 + q;
                    rowcnt[row] = cnt[q];
                    rowcls[row] = c1[q];
                    rowcls[n_nodes + row] = c2[q];
                    rowcls[2 * n_nodes + row] = c3[q];
                }
    }
}

// one wave per graph: lane l adds rows l, l + 64, ... of each class, then the wave's fixed tree
__global__ __launch_bounds__(256) void k_report_graphs(const int64_t* __restrict__ node_off, int64_t n_graphs, int64_t n_nodes,
                                                       int max_nodes, const int32_t* __restrict__ rowcls,
                                                       int64_t* __restrict__ class_pairs) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < n_graphs; g += (int64_t)gridDim.x * 4) {
        int64_t n0;
        int ng;
        stats_graph_range(node_off, (int)g, n_nodes, max_nodes, n0, ng);
        for (int c = 0; c < 3; ++c) {
            unsigned long long s = 0;
            for (int r = lane; r < ng; r += 64) s += (unsigned long long)rowcls[c * n_nodes + n0 + r];
            s = wave_sum_u64(s);
            if (lane == 0) class_pairs[g * 3 + c] = (int64_t)s;
        }
    }
}

// one wave: totals[1 + c] = sum_g class_pairs[g][c]
__global__ __launch_bounds__(64) void k_report_totals(int64_t n_graphs, const int64_t* __restrict__ class_pairs,
                                                      int64_t* __restrict__ totals) {
    for (int c = 0; c < 3; ++c) {
        unsigned long long s = 0;
        for (int64_t g = threadIdx.x; g < n_graphs; g += 64) s += (unsigned long long)class_pairs[g * 3 + c];
        s = wave_sum_u64(s);
        if (threadIdx.x == 0) totals[1 + c] = (int64_t)s;
    }
}

// k_edge_fill's grid, row ownership and entry ids over pred | true; a lane with a set bit also scores its pair.  Ids >=
// edge_capacity are dropped.
__global__ __launch_bounds__(256) void k_report_fill(const float* __restrict__ z, int64_t ld, int D,
                                                     const int64_t* __restrict__ node_off, int64_t n_nodes, int max_nodes,
                                                     int64_t W, DistSigmoid dist_arg,
                                                     const unsigned long long* __restrict__ true_bits,
                                                     const unsigned long long* __restrict__ pred_bits,
                                                     const int32_t* __restrict__ rowptr, int64_t edge_capacity,
                                                     int32_t* __restrict__ senders, int32_t* __restrict__ receivers,
                                                     int32_t* __restrict__ cls, float* __restrict__ score) {
    int64_t n0;
    int ng;
    stats_graph_range(node_off, blockIdx.x, n_nodes, max_nodes, n0, ng);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int words = (ng + 63) / 64;
    const DistSigmoid dist = dist_arg.load();
    for (int i0 = blockIdx.y * kEdgeTile; i0 < ng; i0 += gridDim.y * kEdgeTile) {
        for (int q = 0; q < kEdgeWaveRows; ++q) {
            const int i = i0 + wave * kEdgeWaveRows + q;
            if (i >= ng) break;
            int64_t e0 = rowptr[n0 + i];
            for (int w = 0; w < words && e0 >= 0 && e0 < edge_capacity; ++w) {
                const unsigned long long pw = pred_bits[(n0 + i) * W + w], tw = true_bits[(n0 + i) * W + w];
                const unsigned long long word = pw | tw;
                const int64_t e = e0 + __popcll(word & ((1ull << lane) - 1ull));
                const int j = w * 64 + lane;
                if (((word >> lane) & 1ull) && e < edge_capacity && j < ng) {
                    const float* zr[1] = {z + (n0 + i) * ld};
                    float d2[1];
                    pair_d2(zr, z + (n0 + j) * ld, D, d2);
                    const float a = dist.logit(d2[0]);
                    const bool pr = (pw >> lane) & 1ull, tr = (tw >> lane) & 1ull;
                    senders[e] = (int32_t)(n0 + j);
                    receivers[e] = (int32_t)(n0 + i);
                    cls[e] = pr ? (tr ? 1 : 2) : 3;
                    score[e] = 1.f / (1.f + expf(-a));
                }
                e0 += __popcll(word);
            }
        }
    }
}

struct SelectQ {
    double q[GNF_SELECT_MAX_Q];
};

// the rank-th smallest key (rank < the class's count in [e0, e1)) of the entries of class `want`: four 8-bit digits from the
// top; `prefix` holds the digits found so far.  All lanes of the workgroup call it together and get the key.
__device__ __forceinline__ uint32_t select_kth(const float* __restrict__ score, const int32_t* __restrict__ cls, int64_t e0,
                                               int64_t e1, int want, uint32_t rank, uint32_t* hist, uint32_t* pick) {
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
        __syncthreads();
        for (int64_t e = e0 + threadIdx.x; e < e1; e += kSelectThreads) {
            if (cls[e] != want) continue;
            const uint32_t key = __float_as_uint(score[e]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {   // the scan of the bins: the first whose running total exceeds the rank
            uint32_t cum = 0, bin = 255, left = 0;
            for (uint32_t b = 0; b < 256; ++b) {
                const uint32_t hb = hist[b];
                if (rank < cum + hb) {
                    bin = b;
                    left = rank - cum;
                    break;
                }
                cum += hb;
            }
            pick[0] = bin;
            pick[1] = left;
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        mask |= 255u << shift;
        rank = pick[1];
        __syncthreads();   // pick and hist are rewritten by the next digit
    }
    return prefix;
}

// grid (segment, class index, q index); the q index 0 workgroup also writes the count
__global__ __launch_bounds__(kSelectThreads) void k_score_select(const float* __restrict__ score, const int32_t* __restrict__ cls,
                                                                 const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ seg_nodes, int64_t n_nodes,
                                                                 int64_t edge_capacity, SelectQ Q, int nq,
                                                                 float* __restrict__ stat, int64_t* __restrict__ count) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t pick[2];
    const int64_t s = blockIdx.x;
    const int c = blockIdx.y, k = blockIdx.z;
    int64_t a = seg_nodes[s], b = seg_nodes[s + 1];
    a = a < 0 ? 0 : (a > n_nodes ? n_nodes : a);
    b = b < a ? a : (b > n_nodes ? n_nodes : b);
    int64_t e0 = rowptr[a], e1 = rowptr[b];
    e0 = e0 < 0 ? 0 : (e0 > edge_capacity ? edge_capacity : e0);
    e1 = e1 < e0 ? e0 : (e1 > edge_capacity ? edge_capacity : e1);
    const int want = c + 2;
    if (threadIdx.x == 0) pick[0] = 0u;
    __syncthreads();
    uint32_t mine = 0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += kSelectThreads) mine += cls[e] == want ? 1u : 0u;
    if (mine) atomicAdd(&pick[0], mine);
    __syncthreads();
    const uint32_t n = pick[0];
    __syncthreads();
    if (k == 0 && threadIdx.x == 0) count[s * 2 + c] = (int64_t)n;
    if (k >= nq) return;   // (uniform)
    float* out = stat + ((s * 2 + c) * nq + k) * 2;
    if (n == 0) {
        if (threadIdx.x == 0) out[0] = out[1] = __uint_as_float(0x7fc00000u);
        return;
    }
    double qv = 0.0;
#pragma unroll
    for (int i = 0; i < GNF_SELECT_MAX_Q; ++i)
        if (i == k) qv = Q.q[i];
    const double h = (double)(n - 1u) * qv;   // one fp64 product, as the host forms it
    int64_t lo = (int64_t)floor(h);
    lo = lo < 0 ? 0 : (lo > (int64_t)n - 1 ? (int64_t)n - 1 : lo);
    const int64_t hi = lo + 1 < (int64_t)n ? lo + 1 : (int64_t)n - 1;
    const uint32_t xlo = select_kth(score, cls, e0, e1, want, (uint32_t)lo, hist, pick);
    const uint32_t xhi = hi == lo ? xlo : select_kth(score, cls, e0, e1, want, (uint32_t)hi, hist, pick);
    if (threadIdx.x == 0) {
        out[0] = __uint_as_float(xlo);
        out[1] = __uint_as_float(xhi);
    }
}

static int zero_words(void* p, size_t bytes, hipStream_t st) {
    const size_t words = bytes / sizeof(uint32_t);
    if (!words) return GNF_OK;
    hipLaunchKernelGGL(k_report_zero, dim3(stats_grid((int64_t)((words + 255) / 256))), dim3(256), 0, st, (uint32_t*)p, words);
    GNF_LAUNCH_CHECK("k_report_zero");
    return GNF_OK;
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_adj_report_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_nodes < 0 || max_nodes_per_graph < 0) return 0;
    return report_ws(n_graphs, n_nodes, max_nodes_per_graph).total;
}

int gnf_adj_report_count_f32(const GnfCsr* csr, const GnfDistance* dist, const float* z, int64_t ld, int32_t D,
                             int32_t max_nodes_per_graph, float threshold, int32_t* rowptr, int32_t* n_edge,
                             int64_t* class_pairs, int64_t* totals, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_adj_report_count_f32";
    if (int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kReportMaxNodes, "a row's pair count fits int32")) return rc;
    if (!dist) {
        set_error("%s: null dist", what);
        return GNF_EINVAL;
    }
    if (D < 1 || ld < D) {
        set_error("%s: D=%d ld=%lld", what, D, (long long)ld);
        return GNF_ESHAPE;
    }
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    if (int rc = edge_sizes_ok(what, b, n, max_nodes_per_graph)) return rc;
    if (!rowptr || !totals || (n > 0 && !z) || ((n > 0 || b > 0) && !ws) || (b > 0 && (!n_edge || !class_pairs))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const ReportWs L = report_ws(b, n, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || b == 0) {   // nothing to classify: zeros (n > 0 needs a graph, so n == 0 here)
        if (int rc = zero_words(rowptr, sizeof(int32_t), st)) return rc;
        if (int rc = zero_words(totals, 4 * sizeof(int64_t), st)) return rc;
        if (b > 0) {
            if (int rc = zero_words(n_edge, (size_t)b * sizeof(int32_t), st)) return rc;
            if (int rc = zero_words(class_pairs, (size_t)b * 3 * sizeof(int64_t), st)) return rc;
        }
        return GNF_OK;
    }
    int64_t* node_off = (int64_t*)((char*)ws + L.node_off);
    unsigned long long* true_bits = (unsigned long long*)((char*)ws + L.true_bits);
    unsigned long long* pred_bits = (unsigned long long*)((char*)ws + L.pred_bits);
    int32_t* rowcnt = (int32_t*)((char*)ws + L.rowcnt);
    int32_t* rowcls = (int32_t*)((char*)ws + L.rowcls);
    // the true words (OR atomics), and the counts of rows no tile covers; every offset of the layout is a multiple of 4
    if (int rc = zero_words((char*)ws + L.true_bits, L.total - L.true_bits, st)) return rc;
    hipLaunchKernelGGL(k_report_bitmap, dim3(stats_grid((n + 3) / 4)), dim3(256), 0, st, csr->rowptr, csr->col, n, csr->n_edges,
                       csr->node_offsets, b, max_nodes_per_graph, L.W, true_bits, node_off);
    GNF_LAUNCH_CHECK("k_report_bitmap");
    const DistSigmoid ds = dist_sigmoid(*dist, D);
    const dim3 grid = edge_grid(b, max_nodes_per_graph);
    const size_t row_tile = (size_t)kEdgeTile * D * sizeof(float);
    if (row_tile <= 64 * 1024)
        hipLaunchKernelGGL(k_report_count<true>, grid, dim3(256), row_tile, st, z, ld, D, node_off, n, max_nodes_per_graph, L.W,
                           threshold, ds, true_bits, pred_bits, rowcnt, rowcls);
    else
        hipLaunchKernelGGL(k_report_count<false>, grid, dim3(256), 0, st, z, ld, D, node_off, n, max_nodes_per_graph, L.W,
                           threshold, ds, true_bits, pred_bits, rowcnt, rowcls);
    GNF_LAUNCH_CHECK("k_report_count");
    if (int rc = launch_edge_scan(rowcnt, n, node_off, b, rowptr, n_edge, totals, st)) return rc;
    hipLaunchKernelGGL(k_report_graphs, dim3(stats_grid((b + 3) / 4)), dim3(256), 0, st, node_off, b, n, max_nodes_per_graph,
                       rowcls, class_pairs);
    GNF_LAUNCH_CHECK("k_report_graphs");
    hipLaunchKernelGGL(k_report_totals, dim3(1), dim3(64), 0, st, b, class_pairs, totals);
    GNF_LAUNCH_CHECK("k_report_totals");
    return GNF_OK;
}

int gnf_adj_report_fill(const GnfDistance* dist, const float* z, int64_t ld, int32_t D, int64_t n_graphs, int64_t n_nodes,
                        int32_t max_nodes_per_graph, const int32_t* rowptr, int64_t edge_capacity, int32_t* senders,
                        int32_t* receivers, int32_t* cls, float* score, const void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_adj_report_fill";
    if (!dist) {
        set_error("%s: null dist", what);
        return GNF_EINVAL;
    }
    if (D < 1 || ld < D) {
        set_error("%s: D=%d ld=%lld", what, D, (long long)ld);
        return GNF_ESHAPE;
    }
    if (int rc = edge_sizes_ok(what, n_graphs, n_nodes, max_nodes_per_graph)) return rc;
    if (edge_capacity < 0 || n_graphs > 0x7fffffff || max_nodes_per_graph > kReportMaxNodes) {
        set_error("%s: edge_capacity=%lld n_graphs=%lld max_nodes_per_graph=%d", what, (long long)edge_capacity,
                  (long long)n_graphs, max_nodes_per_graph);
        return GNF_ESHAPE;
    }
    if (!rowptr || !ws || (n_nodes > 0 && !z) || (edge_capacity > 0 && (!senders || !receivers || !cls || !score))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const ReportWs L = report_ws(n_graphs, n_nodes, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    if (n_graphs == 0 || n_nodes == 0 || edge_capacity == 0) return GNF_OK;
    hipLaunchKernelGGL(k_report_fill, edge_grid(n_graphs, max_nodes_per_graph), dim3(256), 0, (hipStream_t)stream, z, ld, D,
                       (const int64_t*)((const char*)ws + L.node_off), n_nodes, max_nodes_per_graph, L.W, dist_sigmoid(*dist, D),
                       (const unsigned long long*)((const char*)ws + L.true_bits),
                       (const unsigned long long*)((const char*)ws + L.pred_bits), rowptr, edge_capacity, senders, receivers,
                       cls, score);
    GNF_LAUNCH_CHECK("k_report_fill");
    return GNF_OK;
}

int gnf_score_select_f32(const float* score, const int32_t* cls, const int32_t* rowptr, const int32_t* seg_nodes, int64_t n_seg,
                         int64_t n_nodes, int64_t edge_capacity, const double* q, int32_t nq, float* stat, int64_t* count,
                         gnf_stream_t stream) {
    const char* what = "gnf_score_select_f32";
    if (n_seg < 0 || n_seg > 0x7fffffff || n_nodes < 0 || edge_capacity < 0 || nq < 0 || nq > GNF_SELECT_MAX_Q) {
        set_error("%s: n_seg=%lld n_nodes=%lld edge_capacity=%lld nq=%d (at most %d)", what, (long long)n_seg, (long long)n_nodes,
                  (long long)edge_capacity, nq, GNF_SELECT_MAX_Q);
        return GNF_ESHAPE;
    }
    // (no segment: stat and count are empty arrays, which a caller may not have an address for)
    if (!rowptr || !seg_nodes || (nq > 0 && !q) || (n_seg > 0 && (!count || (nq > 0 && !stat))) ||
        (edge_capacity > 0 && (!score || !cls))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    SelectQ Q = {};
    for (int i = 0; i < nq; ++i) {
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) {
            set_error("%s: q[%d]=%g (in [0, 1])", what, i, q[i]);
            return GNF_ESHAPE;
        }
        Q.q[i] = q[i];
    }
    if (n_seg == 0) return GNF_OK;
    hipLaunchKernelGGL(k_score_select, dim3((unsigned)n_seg, 2, (unsigned)(nq > 0 ? nq : 1)), dim3(kSelectThreads), 0,
                       (hipStream_t)stream, score, cls, rowptr, seg_nodes, n_nodes, edge_capacity, Q, nq, stat, count);
    GNF_LAUNCH_CHECK("k_score_select");
    return GNF_OK;
}

}  // extern "C"
