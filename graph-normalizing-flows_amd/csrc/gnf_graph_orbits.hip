// Scoring generated graphs on the device, third statistic: the 15 node orbits of the graphlets on 2, 3 and 4 nodes (Przulj's
// numbering, the one ORCA uses) and the MMD of per-graph mean orbit vectors under a Gaussian kernel - next to the degree and
// clustering MMD of gnf_graph_stats.hip the third number GraphRNN-style evaluation reports.  The reference stops at pickling
// the graphs (generate_graphs.py:68-84); nothing in it corresponds to these kernels.
//
// Graph model and bitmap: as in gnf_graph_stats.hip (undirected, simple), built by build_graph_bitmap (gnf_graph_bitmap.h:
// k_stats_bitmap on a zeroed bitmap).  orbit[v][o] = number of INDUCED connected subgraphs on 2..4 nodes that contain v with v in orbit o:
//   0 edge | 1 2 path3 end, middle | 3 triangle | 4 5 path4 end, inner | 6 7 star leaf, centre | 8 4-cycle |
//   9 10 11 tailed triangle: tail end, triangle node of degree 2, of degree 3 | 12 13 chorded 4-cycle: degree 2, 3 | 14 K4
//
// Launches: k_stats_bitmap; k_orbit_degtri (one wave per node, row_degree_triangles as k_stats_nodes: d_k, t_k into the workspace);
// k_orbit_nodes (one wave = one workgroup per node i, row_i in LDS).  All arithmetic is 64-bit integer.
// With c_ik = popc(row_i & row_k), C2(x) = x (x - 1) / 2, C3(x) = x (x - 1) (x - 2) / 6, d = d_i, t = t_i = 1/2 sum_{j in N(i)} c_ij:
//   sweep (lane = a node k != i of the graph, any k):   Q  = sum C2(c_ik)              4-cycles through i
//                                                       X  = sum (d_k - 1) c_ik        walks i - j - k - l, l != j
//         (k in N(i), a bit test on the LDS row):       A  = sum (d_k - 1)   Tn = sum t_k   D2 = sum C2(d_k - 1)
//                                                       P  = sum c_ik (d_k - 2)   E2 = sum C2(c_ik)
//   queue (lane = a neighbour j, 64 at a time, for_each_neighbour; for every k > j in N(i) & N(j)):
//                                                       R  = sum (popc(row_j & row_k) - 1)     triangle i j k + one on edge j k
//                                                       K3 = sum popc(row_i & row_j & row_k)   = 3 * (K4 through i)
// These are NON-INDUCED rooted counts:  n4 = X - 2t, n5 = (d - 1) A - 2t, n6 = D2, n7 = C3(d), n8 = Q, n9 = Tn - 2t, n10 = P,
// n11 = t (d - 2), n12 = R, n13 = E2, n14 = K = K3 / 3.  Each is a fixed integer combination of the induced counts (how often
// the smaller graphlet spans the larger one with the root in place); solved from the densest graphlet down:
//   o14 = K                              o13 = n13 - 3 o14                      o12 = n12 - 3 o14
//   o11 = n11 - 2 o13 - 3 o14            o10 = n10 - 2 o12 - 2 o13 - 6 o14      o9  = n9 - 2 o12 - 3 o14
//   o8  = n8 - o12 - o13 - 3 o14         o7  = n7 - o11 - o13 - o14             o6  = n6 - o9 - o10 - 2 o12 - o13 - 3 o14
//   o5  = n5 - 2 o8 - o10 - 2 o11 - 2 o12 - 4 o13 - 6 o14
//   o4  = n4 - 2 o8 - 2 o9 - o10 - 4 o12 - 2 o13 - 6 o14
//   o3  = t     o2 = C2(d) - t     o1 = A - 2t     o0 = d
// Cost per node: (n_g + sum_{j in N(i)} c_ij) W word operations, W = ceil(max_nodes / 64) - at most (n_g + d_i d_mean) W.
// Every count is below n^3; max_nodes_per_graph <= 8192 keeps them (and the coefficients above) far inside int64.
// Per-graph sums: 64-bit integer atomic adds, order-independent, so the result is deterministic.
//
// Vector MMD.  Sets A [a][L], B [b][L] of int64 sums with int32 counts; row = sums / count in fp64, rows with count <= 0 are
// excluded and counted out; k(x, y) = exp(-|x - y|^2 / (2 sigma^2)).  Workgroup p owns row p: its waves take the rows q of p's
// own set, then (p in A) the rows of B, one wave per pair, both in the same set-relative order, and leave {same-set sum,
// cross sum} in the workspace; one workgroup adds the partials set by set in a fixed set-relative order.  No floating-point
// atomics: two calls give the same bits, and two identical sets give sum AA == sum BB == sum AB bit for bit (MMD^2 == 0).
#include "gnf_graph_bitmap.h"

namespace gnf {

static constexpr int kOrbits = 15;
static constexpr int kOrbitMaxNodes = 8192;

// caller-owned workspace of gnf_graph_orbits (host only): bitmap uint64 [N][W] | gid int32 [N] | deg int32 [N] | tri int32 [N]
struct OrbitWs {
    size_t bitmap, gid, deg, tri, total;
    int64_t W;
};
static OrbitWs orbit_ws(int64_t n_nodes, int32_t max_nodes) {
    OrbitWs L;
    L.W = ((int64_t)max_nodes + 63) / 64;
    L.bitmap = 0;
    L.gid = (size_t)n_nodes * (size_t)L.W * sizeof(uint64_t);
    L.deg = L.gid + (size_t)n_nodes * sizeof(int32_t);
    L.tri = L.deg + (size_t)n_nodes * sizeof(int32_t);
    L.total = (L.tri + (size_t)n_nodes * sizeof(int32_t) + 7) / 8 * 8;
    return L;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) { return (long long)wave_sum_u64((unsigned long long)v); }

// one wave = one workgroup per node: d_i and t_i into the workspace, 0 for a row no graph (or no bitmap column) covers.
// LDS: row_i [W] words | queue [128]
__global__ __launch_bounds__(64) void k_orbit_degtri(const int32_t* __restrict__ off, int64_t n_nodes, int max_nodes, int64_t W,
                                                     const unsigned long long* __restrict__ bitmap,
                                                     const int32_t* __restrict__ gid, int32_t* __restrict__ deg,
                                                     int32_t* __restrict__ tri) {
    extern __shared__ unsigned long long orbit_lds[];
    unsigned long long* row = orbit_lds;        // [W]
    int32_t* queue = (int32_t*)(orbit_lds + W);  // [128]
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < n_nodes; i += gridDim.x) {   // (uniform over the workgroup)
        int g, ng;
        int64_t n0;
        if (!graph_of_row(off, gid, n_nodes, max_nodes, i, g, n0, ng)) {
            if (lane == 0) {
                deg[i] = 0;
                tri[i] = 0;
            }
            continue;
        }
        unsigned long long d, t;
        row_degree_triangles(bitmap, i, row, queue, (ng + 63) / 64, n0, W, d, t);
        if (lane == 0) {
            deg[i] = (int32_t)d;
            tri[i] = (int32_t)t;   // <= C(8191, 2)
        }
    }
}

__device__ __forceinline__ long long choose2(long long x) { return x * (x - 1) / 2; }

// one wave = one workgroup per node.  LDS: row_i [W] words | result [16] int64 | queue [128]
__global__ __launch_bounds__(64) void k_orbit_nodes(const int32_t* __restrict__ off, int64_t n_nodes, int max_nodes, int64_t W,
                                                    const unsigned long long* __restrict__ bitmap,
                                                    const int32_t* __restrict__ gid, const int32_t* __restrict__ deg,
                                                    const int32_t* __restrict__ tri, long long* __restrict__ orbits,
                                                    int64_t ld, unsigned long long* __restrict__ orbit_sums) {
    extern __shared__ unsigned long long orbit_lds[];
    unsigned long long* row = orbit_lds;               // [W]
    long long* result = (long long*)(orbit_lds + W);    // [16]
    int32_t* queue = (int32_t*)(orbit_lds + W + 16);    // [128]
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < n_nodes; i += gridDim.x) {   // (uniform over the workgroup)
        int g, ng;
        int64_t n0;
        if (!graph_of_row(off, gid, n_nodes, max_nodes, i, g, n0, ng)) {   // zeros, no share in a sum
            if (lane < kOrbits) orbits[i * ld + lane] = 0;
            continue;
        }
        const int64_t li = i - n0;
        const int words = (ng + 63) / 64;
        __syncthreads();   // the previous node's readers are done
        for (int w = lane; w < words; w += 64) row[w] = bitmap[i * W + w];
        __syncthreads();
        // sweep: every node k != i of the graph, c_ik against the LDS row
        long long d = 0, t2 = 0, Q = 0, X = 0, A = 0, Tn = 0, D2 = 0, P = 0, E2 = 0;
        for (int k = lane; k < ng; k += 64) {
            if (k == (int)li) continue;
            const unsigned long long* rk = bitmap + (n0 + k) * W;
            long long c = 0;
            for (int w = 0; w < words; ++w) c += __popcll(row[w] & rk[w]);
            const long long dk = deg[n0 + k];
            Q += choose2(c);
            X += (dk - 1) * c;   // (c <= d_k: a node without neighbours adds 0)
            if ((row[k >> 6] >> (k & 63)) & 1ull) {
                d += 1;
                t2 += c;
                A += dk - 1;
                Tn += tri[n0 + k];
                D2 += choose2(dk - 1);
                P += c * (dk - 2);   // (c <= d_k - 1 here)
                E2 += choose2(c);
            }
        }
        d = wave_sum_i64(d), t2 = wave_sum_i64(t2), Q = wave_sum_i64(Q), X = wave_sum_i64(X), A = wave_sum_i64(A);
        Tn = wave_sum_i64(Tn), D2 = wave_sum_i64(D2), P = wave_sum_i64(P), E2 = wave_sum_i64(E2);
        // queue: every neighbour j, then every k > j of N(i) & N(j) - the triangles i j k, each once
        long long R = 0, K3 = 0;
        for_each_neighbour(row, queue, words, lane, [&](int lj) {
            const unsigned long long* rj = bitmap + (n0 + lj) * W;
            for (int w = lj >> 6; w < words; ++w) {
                unsigned long long m = row[w] & rj[w];
                if (w == (lj >> 6)) m &= ~((2ull << (lj & 63)) - 1ull);   // columns above lj (bit 63: nothing left)
                while (m) {
                    const int k = w * 64 + __ffsll((long long)m) - 1;
                    m &= m - 1ull;
                    const unsigned long long* rk = bitmap + (n0 + k) * W;
                    long long cjk = 0;
                    for (int w2 = 0; w2 < words; ++w2) {
                        const unsigned long long jk = rj[w2] & rk[w2];
                        cjk += __popcll(jk);
                        K3 += __popcll(jk & row[w2]);
                    }
                    R += cjk - 1;
                }
            }
        });
        R = wave_sum_i64(R), K3 = wave_sum_i64(K3);
        if (lane == 0) {
            const long long t = t2 / 2, K = K3 / 3;
            long long o[kOrbits];
            o[14] = K;
            o[13] = E2 - 3 * K;
            o[12] = R - 3 * K;
            o[11] = t * (d - 2) - 2 * o[13] - 3 * K;
            o[10] = P - 2 * o[12] - 2 * o[13] - 6 * K;
            o[9] = (Tn - 2 * t) - 2 * o[12] - 3 * K;
            o[8] = Q - o[12] - o[13] - 3 * K;
            o[7] = d * (d - 1) * (d - 2) / 6 - o[11] - o[13] - K;
            o[6] = D2 - o[9] - o[10] - 2 * o[12] - o[13] - 3 * K;
            o[5] = ((d - 1) * A - 2 * t) - 2 * o[8] - o[10] - 2 * o[11] - 2 * o[12] - 4 * o[13] - 6 * K;
            o[4] = (X - 2 * t) - 2 * o[8] - 2 * o[9] - o[10] - 4 * o[12] - 2 * o[13] - 6 * K;
            o[3] = t;
            o[2] = choose2(d) - t;
            o[1] = A - 2 * t;
            o[0] = d;
#pragma unroll
            for (int c = 0; c < kOrbits; ++c) result[c] = o[c];
        }
        __syncthreads();
        if (lane < kOrbits) {
            const long long v = result[lane];
            orbits[i * ld + lane] = v;
            atomicAdd(&orbit_sums[(int64_t)g * kOrbits + lane], (unsigned long long)v);   // (counts: never negative)
        }
    }
}

// ---- vector MMD ------------------------------------------------------------------------------------------------------------
// workspace (host only): partials double [a + b][2] = {sum over p's own set, sum over the other set (rows of A only)}
struct VecSets {
    const long long *xa, *xb;
    const int32_t *ca, *cb;
    int64_t a, b, lda, ldb;
    int32_t L;
};

// sum over the rows q of one set of k(row p, row q); wave w takes q = w, w + 4, ...
__device__ __forceinline__ double vecmmd_row_against(const long long* __restrict__ xp, double np, const long long* __restrict__ xs,
                                                     const int32_t* __restrict__ cs, int64_t rows, int64_t lds, int L,
                                                     double neg_half_inv_sigma2, int lane, int wave) {
    double acc = 0.0;
    for (int64_t q = wave; q < rows; q += 4) {
        const int32_t cq = cs[q];
        if (cq <= 0) continue;
        const double nq = (double)cq;
        const long long* xq = xs + q * lds;
        double part = 0.0;
        for (int c0 = 0; c0 < L; c0 += 64) {
            const int i = c0 + lane;
            if (i < L) {
                const double v = (double)xp[i] / np - (double)xq[i] / nq;
                part += v * v;
            }
        }
        acc += exp(wave_sum_f64(part) * neg_half_inv_sigma2);
    }
    return acc;
}

__global__ __launch_bounds__(256) void k_vecmmd_pairs(VecSets s, double neg_half_inv_sigma2, double* __restrict__ partials) {
    __shared__ double sh[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = blockIdx.x;
    const bool in_a = p < s.a;
    const long long* xp = in_a ? s.xa + p * s.lda : s.xb + (p - s.a) * s.ldb;
    const int32_t cp = in_a ? s.ca[p] : s.cb[p - s.a];
    double same = 0.0, cross = 0.0;
    if (cp > 0) {
        const double np = (double)cp;
        if (in_a) {
            same = vecmmd_row_against(xp, np, s.xa, s.ca, s.a, s.lda, s.L, neg_half_inv_sigma2, lane, wave);
            cross = vecmmd_row_against(xp, np, s.xb, s.cb, s.b, s.ldb, s.L, neg_half_inv_sigma2, lane, wave);
        } else {
            same = vecmmd_row_against(xp, np, s.xb, s.cb, s.b, s.ldb, s.L, neg_half_inv_sigma2, lane, wave);
        }
    }
    if (lane == 0) {
        sh[wave][0] = same;
        sh[wave][1] = cross;
    }
    __syncthreads();
    if (threadIdx.x < 2) partials[p * 2 + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// one workgroup: out5 = {sum AA, sum BB, sum AB, cnt_a, cnt_b}; thread t adds up rows t, t + 256, ... OF EACH SET in that
// order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void k_vecmmd_final(int64_t a, int64_t b, const int32_t* __restrict__ ca,
                                                      const int32_t* __restrict__ cb, const double* __restrict__ partials,
                                                      double* __restrict__ out5) {
    __shared__ double sh[5][256];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r = threadIdx.x; r < a; r += 256) {
        v[0] += partials[r * 2];
        v[2] += partials[r * 2 + 1];
        if (ca[r] > 0) v[3] += 1.0;
    }
    for (int64_t r = threadIdx.x; r < b; r += 256) {
        v[1] += partials[(a + r) * 2];
        if (cb[r] > 0) v[4] += 1.0;
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

size_t gnf_graph_orbits_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_nodes < 0 || max_nodes_per_graph < 0) return 0;
    return orbit_ws(n_nodes, max_nodes_per_graph).total;
}

int gnf_graph_orbits(const GnfCsr* csr, int32_t max_nodes_per_graph, int64_t* orbits, int64_t ld_orbits, int64_t* orbit_sums,
                     void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_graph_orbits";
    if (int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kOrbitMaxNodes, "the cost per node grows with n_g + d_i d_mean"))
        return rc;
    if (ld_orbits < kOrbits) {
        set_error("%s: ld_orbits=%lld (ld_orbits >= %d)", what, (long long)ld_orbits, kOrbits);
        return GNF_ESHAPE;
    }
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    if ((n > 0 && (!orbits || !ws)) || (b > 0 && !orbit_sums)) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const OrbitWs L = orbit_ws(n, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    if (b == 0) return GNF_OK;   // an empty batch: nothing to write
    hipStream_t st = (hipStream_t)stream;
    GNF_HIP_TRY(hipMemsetAsync(orbit_sums, 0, (size_t)b * kOrbits * sizeof(int64_t), st));
    if (n == 0) return GNF_OK;
    unsigned long long* bitmap = (unsigned long long*)((char*)ws + L.bitmap);
    int32_t* gid = (int32_t*)((char*)ws + L.gid);
    int32_t* deg = (int32_t*)((char*)ws + L.deg);
    int32_t* tri = (int32_t*)((char*)ws + L.tri);
    if (int rc = build_graph_bitmap(csr, max_nodes_per_graph, L.W, bitmap, gid, st)) return rc;
    const size_t lds = (size_t)L.W * sizeof(uint64_t) + 128 * sizeof(int32_t);   // <= 1.5 KB
    hipLaunchKernelGGL(k_orbit_degtri, dim3(stats_grid(n)), dim3(64), lds, st, csr->node_offsets, n, max_nodes_per_graph, L.W,
                       bitmap, gid, deg, tri);
    GNF_LAUNCH_CHECK("k_orbit_degtri");
    hipLaunchKernelGGL(k_orbit_nodes, dim3(stats_grid(n)), dim3(64), lds + 16 * sizeof(int64_t), st, csr->node_offsets, n,
                       max_nodes_per_graph, L.W, bitmap, gid, deg, tri, (long long*)orbits, ld_orbits,
                       (unsigned long long*)orbit_sums);
    GNF_LAUNCH_CHECK("k_orbit_nodes");
    return GNF_OK;
}

size_t gnf_vec_mmd_workspace_bytes(int64_t a, int64_t b) {
    if (a < 0 || b < 0) return 0;
    return (size_t)(a + b) * 2 * sizeof(double);
}

int gnf_vec_mmd_i64(const int64_t* xa, const int32_t* count_a, int64_t a, int64_t lda, const int64_t* xb,
                    const int32_t* count_b, int64_t b, int64_t ldb, int32_t L, double sigma, double* out5, void* ws,
                    size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_vec_mmd_i64";
    if (a < 0 || b < 0 || L < 0 || L > lda || L > ldb || a + b > 0x7fffffff) {
        set_error("%s: a=%lld lda=%lld b=%lld ldb=%lld L=%d", what, (long long)a, (long long)lda, (long long)b, (long long)ldb, L);
        return GNF_ESHAPE;
    }
    if (!(sigma > 0.0)) {
        set_error("%s: sigma=%g must be positive", what, sigma);
        return GNF_EINVAL;
    }
    if (!out5 || (a > 0 && (!count_a || (L > 0 && !xa))) || (b > 0 && (!count_b || (L > 0 && !xb))) || (a + b > 0 && !ws)) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const size_t need = gnf_vec_mmd_workspace_bytes(a, b);
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
    const VecSets s = {(const long long*)xa, (const long long*)xb, count_a, count_b, a, b, lda, ldb, L};
    double* partials = (double*)ws;
    hipLaunchKernelGGL(k_vecmmd_pairs, dim3((unsigned)n), dim3(256), 0, st, s, -0.5 / (sigma * sigma), partials);
    GNF_LAUNCH_CHECK("k_vecmmd_pairs");
    hipLaunchKernelGGL(k_vecmmd_final, dim3(1), dim3(256), 0, st, a, b, count_a, count_b, partials, out5);
    GNF_LAUNCH_CHECK("k_vecmmd_final");
    return GNF_OK;
}

}  // extern "C"
