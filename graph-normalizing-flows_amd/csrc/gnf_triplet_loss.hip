// Sampled triplet loss of embeddings against a true batch (include/gnf_triplet_loss.h): triplet_loss of the reference
// (loss.py:221-270) and dL/dnodes, from the sender-grouped CSR, without the dense [N, N] true_adj / inv_true_adj / distances
// matrices the reference builds, normalises and samples from.  The workspace is O(N * L); there is no global bitmap.
//
// k_triplet_sample.  One wave (a workgroup of 64) per node i.
//   The out-row bitmap of i (one bit per graph-local column) is built in LDS from i's CSR row with 64-bit integer OR; entries
//   outside the graph's window are dropped, self loops too under GNF_TRIPLET_SELF_SKIP; bit i is then set, so that the unset
//   bits below ng are the negative candidates.  The ballots of the valid entries give the positive count; per-lane popcounts
//   of the inverted words and a wave prefix scan give the negative count and, in LDS, the exclusive prefix per word.
//   Selection: lane l owns round l (L <= 64).  Its positive is the k-th valid entry, found in one more walk over the row (the
//   chunk's ballot is uniform: every lane looks for its own k in it); its negative is the k-th unset bit, by binary search on
//   the prefix and a rank-select inside the word.
//   Scores: the same lane walks the features in ascending order for its two pairs - the fmaf chain of gnf_pred_adj_f32, so d2
//   has that entry point's bits - then the score, the term and per pair the coefficient dterm/dscore * dscore/d(d2 or dot).
//   It stores (j, coefficient) as records 2 l (positive) and 2 l + 1 (negative) of row i; the row's terms are added in fp64
//   through the wave's fixed tree.
// k_triplet_graphs.  One wave per graph: adds the rows' fp64 sums and skipped counts in a fixed order.  With a gradient it
//   also groups the graph's records by the node they chose - a stable counting sort by one wave, 64 records at a time in
//   ascending record id: count, prefix scan, fill.  A lane's slot is the destination's cursor plus the number of lower lanes of
//   the chunk with the same destination, so every bucket lists its records in ascending id: no atomics, nothing to sort.
// k_triplet_grad.  One wave per row j, lanes along the features: its own 2 L records in loop order, then its bucket in order.
// k_triplet_total.  One wave over the graphs.
// No floating-point atomics: two calls on the same input give the same bits.  Every loop is bounded by the graph's size, the
// row's length or 2 L.
#include "gnf_distance_dev.h"
#include "gnf_graph_bitmap.h"

namespace gnf {

static constexpr int kTripletMaxNodes = GNF_TRIPLET_MAX_NODES;
static constexpr int kTripletMaxLoops = GNF_TRIPLET_MAX_LOOPS;

// caller-owned workspace (host only): chosen node int32 [N][2L] | coefficient float [N][2L] | records by chosen node int32
// [N][2L] | row loss double [N] | row skipped int32 [N] | incoming count int32 [N] | first int32 [N] | cursor int32 [N]
struct TripletWs {
    size_t rec_j, rec_c, bucket, row_loss, row_skip, cnt, first, cursor, total;
};
inline TripletWs triplet_ws(int64_t n_nodes, int32_t loops) {
    TripletWs L;
    const size_t rec = (size_t)n_nodes * 2 * (size_t)loops * sizeof(int32_t), row = (size_t)n_nodes * sizeof(int32_t);
    L.rec_j = 0;
    L.rec_c = rec;
    L.bucket = 2 * rec;
    L.row_loss = 3 * rec;   // (a multiple of 8: rec is one of 8)
    L.row_skip = L.row_loss + (size_t)n_nodes * sizeof(double);
    L.cnt = L.row_skip + row;
    L.first = L.cnt + row;
    L.cursor = L.first + row;
    L.total = (L.cursor + row + 7) / 8 * 8;
    return L;
}

struct TripletParams {
    int score, loss, loops, skip_self;
    float temp, shift, scale, margin;
    unsigned long long seed;
};

// the draw of (seed, l, which, i) without a `draws` tensor: DEFINED in include/gnf_triplet_loss.h
__device__ __forceinline__ unsigned long long triplet_hash(unsigned long long seed, int l, int which, long long i) {
    unsigned long long x = seed ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1)) ^
                           (0xBF58476D1CE4E5B9ull * (unsigned long long)(2 * l + which + 1));
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x >> 32;
}

// position of the k-th (from 0) set bit of m; k < popcount(m)
__device__ __forceinline__ int select64(unsigned long long m, int k) {
    int pos = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int c = __popcll((m >> pos) & ((1ull << s) - 1ull));
        if (k >= c) {
            k -= c;
            pos += s;
        }
    }
    return pos;
}

// the columns of word w that lie below ng
__device__ __forceinline__ unsigned long long word_mask(int w, int ng) {
    const int left = ng - w * 64;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// score s(x) and ds/dx, x = d2 or dot
__device__ __forceinline__ void triplet_score(const TripletParams& P, float x, float& s, float& ds) {
    constexpr float kInvPi = 0.31830988618379067f;
    switch (P.score) {
        case GNF_TRIPLET_L2:
        case GNF_TRIPLET_DOT:
            s = x;
            ds = 1.f;
            break;
        case GNF_TRIPLET_EXP_L2:
            s = expf(-x);
            ds = -s;
            break;
        case GNF_TRIPLET_SIGMOID_L2: {
            const float u = sigmoid_l2_logit(P.temp, P.shift, P.scale, x);
            s = 1.f / (1.f + expf(-u));
            ds = -(P.temp * P.scale) * (s * (1.f - s));
            break;
        }
        case GNF_TRIPLET_HACKY_CAUCHY_L2: {
            const float a = -(x - 4.f);
            s = kInvPi * atanf(a) + 0.5f;
            ds = -kInvPi / (1.f + a * a);
            break;
        }
        default: {   // GNF_TRIPLET_SIGMOID_DOT
            s = 1.f / (1.f + expf(-(x - 0.5f)));
            ds = s * (1.f - s);
            break;
        }
    }
}

// LDS: row uint64 [words_lds] | pref int32 [words_lds]
__global__ __launch_bounds__(64) void k_triplet_sample(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                       int64_t n_nodes, int64_t n_edges, const int32_t* __restrict__ off,
                                                       int64_t n_graphs, int max_nodes, int words_lds,
                                                       const float* __restrict__ z, int64_t ld, int D, TripletParams P,
                                                       const uint32_t* __restrict__ draws, int32_t* __restrict__ rec_j,
                                                       float* __restrict__ rec_c, double* __restrict__ row_loss,
                                                       int32_t* __restrict__ row_skip, float* __restrict__ loss_per_node,
                                                       int32_t* __restrict__ pos_index, int32_t* __restrict__ neg_index) {
    extern __shared__ unsigned long long trip_lds[];
    unsigned long long* row = trip_lds;
    int32_t* pref = (int32_t*)(row + words_lds);
    const int lane = threadIdx.x;
    const int L = P.loops;
    const bool is_dot = P.score == GNF_TRIPLET_DOT || P.score == GNF_TRIPLET_SIGMOID_DOT;
    for (int64_t i = blockIdx.x; i < n_nodes; i += gridDim.x) {   // (everything up to the lane's own round is uniform)
        const int g = stats_graph_of(off, n_graphs, i);
        int64_t n0 = 0;
        int ng = 0;
        if (g >= 0) stats_graph_range(off, g, n_nodes, max_nodes, n0, ng);
        const int64_t li64 = i - n0;
        const int64_t rec0 = i * 2 * L;
        if (g < 0 || li64 < 0 || li64 >= ng) {   // a row in no graph: no terms
            if (lane < L) {
                rec_j[rec0 + 2 * lane] = rec_j[rec0 + 2 * lane + 1] = -1;
                rec_c[rec0 + 2 * lane] = rec_c[rec0 + 2 * lane + 1] = 0.f;
                if (pos_index) pos_index[(int64_t)lane * n_nodes + i] = -1;
                if (neg_index) neg_index[(int64_t)lane * n_nodes + i] = -1;
            }
            if (lane == 0) {
                row_loss[i] = 0.0;
                row_skip[i] = 0;
                loss_per_node[i] = 0.f;
            }
            continue;
        }
        const int li = (int)li64;
        const int words = (ng + 63) >> 6;   // <= words_lds: ng <= max_nodes
        __syncthreads();                    // the previous node's readers are done
        for (int w = lane; w < words; w += 64) row[w] = 0ull;
        __syncthreads();
        int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > n_edges) e1 = n_edges;
        unsigned long long pcnt = 0;   // valid entries of the row, with multiplicity
        for (int64_t eb = e0; eb < e1; eb += 64) {
            const int64_t e = eb + lane;
            bool valid = false;
            if (e < e1) {
                const int64_t lj = (int64_t)col[e] - n0;
                valid = lj >= 0 && lj < ng && !(P.skip_self && lj == li);
                if (valid) atomicOr(&row[lj >> 6], 1ull << (lj & 63));
            }
            pcnt += (unsigned long long)__popcll(__ballot(valid));
        }
        __syncthreads();
        if (lane == 0) row[li >> 6] |= 1ull << (li & 63);   // i itself is no negative
        __syncthreads();
        int run = 0;   // unset columns so far
        for (int w0 = 0; w0 < words; w0 += 64) {
            const int w = w0 + lane;
            const int c = w < words ? __popcll(~row[w] & word_mask(w, ng)) : 0;
            const int incl = wave_incl_scan(c, lane);
            if (w < words) pref[w] = run + incl - c;
            run += __shfl(incl, 63, 64);
        }
        const unsigned long long ncnt = (unsigned long long)run;
        __syncthreads();
        const bool has = lane < L && pcnt > 0 && ncnt > 0;
        unsigned long long kp = 0, kn = 0;
        if (has) {
            const unsigned long long rp = draws ? (unsigned long long)draws[((int64_t)lane * 2 + 0) * n_nodes + i]
                                                : triplet_hash(P.seed, lane, 0, i);
            const unsigned long long rn = draws ? (unsigned long long)draws[((int64_t)lane * 2 + 1) * n_nodes + i]
                                                : triplet_hash(P.seed, lane, 1, i);
            kp = (rp * pcnt) >> 32;
            kn = (rn * ncnt) >> 32;
        }
        // ---- the kp-th valid entry: one more walk over the row
        int64_t esel = -1;
        if (pcnt > 0 && ncnt > 0) {   // (uniform)
            unsigned long long base = 0;
            for (int64_t eb = e0; eb < e1; eb += 64) {
                const int64_t e = eb + lane;
                bool valid = false;
                if (e < e1) {
                    const int64_t lj = (int64_t)col[e] - n0;
                    valid = lj >= 0 && lj < ng && !(P.skip_self && lj == li);
                }
                const unsigned long long m = __ballot(valid);
                const unsigned long long c = (unsigned long long)__popcll(m);
                if (has && esel < 0 && kp < base + c) esel = eb + select64(m, (int)(kp - base));
                base += c;
            }
        }
        int64_t jp = -1, jn = -1;
        float p = 0.f, q = 0.f, cp = 0.f, cq = 0.f, term = 0.f;
        bool kept = false;
        if (has && esel >= 0) {
            jp = col[esel];
            // ---- the kn-th unset column: the last word whose prefix is <= kn holds it
            int lo = 0, hi = words;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((unsigned long long)pref[mid] <= kn) lo = mid; else hi = mid;
            }
            const unsigned long long inv = ~row[lo] & word_mask(lo, ng);
            int k = (int)(kn - (unsigned long long)pref[lo]);
            const int c = __popcll(inv);
            if (k >= c) k = c - 1;   // (cannot happen; keeps select64 inside the word)
            jn = n0 + (int64_t)lo * 64 + (c > 0 ? select64(inv, k) : 0);
            if (jn >= n0 + ng) jn = n0 + ng - 1;
            // ---- both scores: the features in ascending order
            const float* zi = z + i * ld;
            const float* za = z + jp * ld;
            const float* zb = z + jn * ld;
            float xp = 0.f, xq = 0.f;
            for (int f = 0; f < D; ++f) {
                const float v = zi[f], a = za[f], b = zb[f];
                if (is_dot) {
                    xp = fmaf(v, a, xp);
                    xq = fmaf(v, b, xq);
                } else {
                    const float da = v - a, db = v - b;
                    xp = fmaf(da, da, xp);
                    xq = fmaf(db, db, xq);
                }
            }
            float dp, dq;
            triplet_score(P, xp, p, dp);
            triplet_score(P, xq, q, dq);
            if (jp == i) p = 0.f, dp = 0.f;   // the diagonal of `distances` is zeroed
            if (P.loss == GNF_TRIPLET_MARGIN) {
                const float t = (P.margin - p) + q;
                kept = true;
                if (t > 0.f) {
                    term = t;
                    cp = -dp;
                    cq = dq;
                }
            } else {
                const float s = p + q;
                if (s != 0.f) {
                    kept = true;
                    term = p / s;
                    cp = ((q / s) / s) * dp;   // (s * s may underflow where s does not)
                    cq = -((p / s) / s) * dq;
                }
            }
            if (!kept) jp = jn = -1;
        }
        if (lane < L) {
            rec_j[rec0 + 2 * lane] = (int32_t)jp;
            rec_j[rec0 + 2 * lane + 1] = (int32_t)jn;
            rec_c[rec0 + 2 * lane] = cp;
            rec_c[rec0 + 2 * lane + 1] = cq;
            if (pos_index) pos_index[(int64_t)lane * n_nodes + i] = (int32_t)jp;
            if (neg_index) neg_index[(int64_t)lane * n_nodes + i] = (int32_t)jn;
        }
        const double rl = wave_sum_f64(kept ? (double)term : 0.0);
        const unsigned long long sk = wave_sum_u64(lane < L && !kept ? 1ull : 0ull);
        if (lane == 0) {
            row_loss[i] = rl;
            row_skip[i] = (int32_t)sk;
            loss_per_node[i] = (float)rl;
        }
    }
}

// among the 64 lanes' keys (key < 0: none): rank = lower lanes with the same key, mult = lanes with it
__device__ __forceinline__ void chunk_rank(int key, int lane, int& rank, int& mult) {
    rank = mult = 0;
    for (int s = 0; s < 64; ++s) {
        const int ks = __shfl(key, s, 64);
        if (ks == key) {
            ++mult;
            if (s < lane) ++rank;
        }
    }
}

// one wave per graph.  index: also group the graph's records by chosen node (cnt / first / cursor [N], bucket [N][2L])
__global__ __launch_bounds__(64) void k_triplet_graphs(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes,
                                                       int max_nodes, int L, const double* __restrict__ row_loss,
                                                       const int32_t* __restrict__ row_skip,
                                                       double* __restrict__ loss_per_graph, int64_t* __restrict__ skipped_terms,
                                                       int index, const int32_t* __restrict__ rec_j,
                                                       const float* __restrict__ rec_c, int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ first, int32_t* __restrict__ cursor,
                                                       int32_t* __restrict__ bucket) {
    const int lane = threadIdx.x;
    const int64_t total = n_nodes * 2 * L;   // <= INT32_MAX (checked on the host)
    for (int64_t g = blockIdx.x; g < n_graphs; g += gridDim.x) {
        int64_t n0;
        int ng;
        stats_graph_range(off, (int)g, n_nodes, max_nodes, n0, ng);
        double l = 0.0;
        unsigned long long s = 0;
        for (int r = lane; r < ng; r += 64) {
            l += row_loss[n0 + r];
            s += (unsigned long long)row_skip[n0 + r];
        }
        l = wave_sum_f64(l);
        s = wave_sum_u64(s);
        if (lane == 0) {
            loss_per_graph[g] = l;
            skipped_terms[g] = (int64_t)s;
        }
        if (!index) continue;   // (uniform)
        for (int r = lane; r < ng; r += 64) cnt[n0 + r] = 0;
        __syncthreads();
        const int nrec = ng * 2 * L;        // <= 65536 * 128
        const int64_t base = n0 * 2 * L;
        for (int pass = 0; pass < 2; ++pass) {
            for (int c0 = 0; c0 < nrec; c0 += 64) {
                const int q = c0 + lane;
                int key = -1;
                if (q < nrec) {
                    const int64_t j = rec_j[base + q];
                    if (j >= n0 && j < n0 + ng && j != n0 + q / (2 * L) && rec_c[base + q] != 0.f) key = (int)(j - n0);
                }
                int rank, mult;
                chunk_rank(key, lane, rank, mult);
                if (key >= 0) {
                    if (pass == 0) {
                        if (rank == 0) cnt[n0 + key] += mult;   // (one lane per destination and chunk)
                    } else {
                        const int cur = cursor[n0 + key];
                        const int64_t pos = (int64_t)cur + rank;
                        if (pos >= 0 && pos < total) bucket[pos] = (int32_t)(base + q);
                        if (rank == 0) cursor[n0 + key] = cur + mult;
                    }
                }
                __syncthreads();   // the next chunk reads what this one wrote
            }
            if (pass == 0) {
                int run = 0;
                for (int r0 = 0; r0 < ng; r0 += 64) {
                    const int r = r0 + lane;
                    const int c = r < ng ? cnt[n0 + r] : 0;
                    const int incl = wave_incl_scan(c, lane);
                    if (r < ng) first[n0 + r] = cursor[n0 + r] = (int32_t)(base + run + incl - c);
                    run += __shfl(incl, 63, 64);
                }
                __syncthreads();
            }
        }
    }
}

// one wave per row j, lanes along the features
__global__ __launch_bounds__(64) void k_triplet_grad(const float* __restrict__ z, int64_t ld, int D,
                                                     const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes,
                                                     int max_nodes, int L, int is_dot, const int32_t* __restrict__ rec_j,
                                                     const float* __restrict__ rec_c, const int32_t* __restrict__ cnt,
                                                     const int32_t* __restrict__ first, const int32_t* __restrict__ bucket,
                                                     float* __restrict__ grad, int64_t ldg, float grad_scale) {
    const int lane = threadIdx.x;
    const int64_t total = n_nodes * 2 * L;
    for (int64_t j = blockIdx.x; j < n_nodes; j += gridDim.x) {
        const int g = stats_graph_of(off, n_graphs, j);
        int64_t n0 = 0;
        int ng = 0;
        if (g >= 0) stats_graph_range(off, g, n_nodes, max_nodes, n0, ng);
        if (g < 0 || j - n0 < 0 || j - n0 >= ng) {   // a row in no graph: its gradient is zero
            for (int f = lane; f < D; f += 64) grad[j * ldg + f] = 0.f;
            continue;
        }
        int64_t b0 = first[j], b1 = b0 + cnt[j];
        if (b0 < 0) b0 = 0;
        if (b1 > total) b1 = total;
        const int64_t own = j * 2 * L;
        for (int f0 = 0; f0 < D; f0 += 64) {
            const int f = f0 + lane;
            if (f >= D) continue;   // (no wave-wide operation below)
            const float zj = z[j * ld + f];
            float acc = 0.f;
            for (int r = 0; r < 2 * L; ++r) {
                const int64_t o = rec_j[own + r];
                const float c = rec_c[own + r];
                if (o < 0 || o >= n_nodes || o == j || c == 0.f) continue;   // skipped, the diagonal, an inactive hinge
                const float zo = z[o * ld + f];
                acc = is_dot ? fmaf(c, zo, acc) : fmaf(2.f * c, zj - zo, acc);
            }
            for (int64_t b = b0; b < b1; ++b) {
                const int64_t rid = bucket[b];
                if (rid < 0 || rid >= total) continue;
                const float c = rec_c[rid];
                if (c == 0.f) continue;
                const float zo = z[(rid / (2 * L)) * ld + f];
                acc = is_dot ? fmaf(c, zo, acc) : fmaf(2.f * c, zj - zo, acc);
            }
            grad[j * ldg + f] = acc * grad_scale;
        }
    }
}

// one wave: sums2 = { sum_g loss_per_graph[g], that / kept terms }
__global__ __launch_bounds__(64) void k_triplet_total(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes,
                                                      int max_nodes, int L, const double* __restrict__ loss_per_graph,
                                                      const int64_t* __restrict__ skipped_terms, double* __restrict__ sums2) {
    double l = 0.0;
    unsigned long long kept = 0;
    for (int64_t g = threadIdx.x; g < n_graphs; g += 64) {
        int64_t n0;
        int ng;
        stats_graph_range(off, (int)g, n_nodes, max_nodes, n0, ng);
        l += loss_per_graph[g];
        kept += (unsigned long long)((int64_t)ng * L - skipped_terms[g]);
    }
    l = wave_sum_f64(l);
    kept = wave_sum_u64(kept);
    if (threadIdx.x == 0) {
        sums2[0] = l;
        sums2[1] = kept == 0 ? 0.0 : l / (double)kept;
    }
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_triplet_loss_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t num_sampling_loops) {
    if (n_graphs < 0 || n_nodes < 0 || num_sampling_loops < 1 || num_sampling_loops > kTripletMaxLoops) return 0;
    if (n_nodes * 2 * num_sampling_loops > 0x7fffffffLL) return 0;
    return triplet_ws(n_nodes, num_sampling_loops).total;
}

int gnf_triplet_loss_f32(const GnfCsr* csr, const float* z, int64_t ld, int32_t D, int32_t max_nodes_per_graph,
                         const GnfTripletSpec* spec, const uint32_t* draws, float* loss_per_node, double* loss_per_graph,
                         double* sums2, int64_t* skipped_terms, int32_t* pos_index, int32_t* neg_index, float* grad,
                         int64_t ld_grad, float grad_scale, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_triplet_loss_f32";
    if (!csr || !spec) {
        set_error("%s: null %s", what, csr ? "spec" : "csr_t");
        return GNF_EINVAL;
    }
    if (spec->score < GNF_TRIPLET_L2 || spec->score > GNF_TRIPLET_SIGMOID_DOT ||
        (spec->loss != GNF_TRIPLET_MARGIN && spec->loss != GNF_TRIPLET_RELATIVE) ||
        (spec->self_loops != GNF_TRIPLET_SELF_KEEP && spec->self_loops != GNF_TRIPLET_SELF_SKIP)) {
        set_error("%s: score=%d loss=%d self_loops=%d", what, spec->score, spec->loss, spec->self_loops);
        return GNF_EINVAL;
    }
    if (D < 1 || ld < D || (grad && ld_grad < D)) {
        set_error("%s: D=%d ld=%lld ld_grad=%lld", what, D, (long long)ld, (long long)ld_grad);
        return GNF_ESHAPE;
    }
    if (spec->num_sampling_loops < 1 || spec->num_sampling_loops > kTripletMaxLoops) {
        set_error("%s: num_sampling_loops=%d (1 <= num_sampling_loops <= %d)", what, spec->num_sampling_loops, kTripletMaxLoops);
        return GNF_ESHAPE;
    }
    const int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kTripletMaxNodes, "a row's bitmap is held in LDS");
    if (rc != GNF_OK) return rc;
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    const int L = spec->num_sampling_loops;
    if (n * 2 * L > 0x7fffffffLL) {
        set_error("%s: n_nodes=%lld with num_sampling_loops=%d (n_nodes * 2 L <= INT32_MAX)", what, (long long)n, L);
        return GNF_ESHAPE;
    }
    if (!sums2 || (n > 0 && (!z || !ws || !loss_per_node)) || (b > 0 && (!loss_per_graph || !skipped_terms))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const TripletWs W = triplet_ws(n, L);
    if (ws_bytes < W.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, W.total);
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || b == 0) {   // nothing to score: zeros
        GNF_HIP_TRY(hipMemsetAsync(sums2, 0, 2 * sizeof(double), st));
        if (b > 0) {
            GNF_HIP_TRY(hipMemsetAsync(loss_per_graph, 0, (size_t)b * sizeof(double), st));
            GNF_HIP_TRY(hipMemsetAsync(skipped_terms, 0, (size_t)b * sizeof(int64_t), st));
        }
        return GNF_OK;
    }
    int32_t* rec_j = (int32_t*)((char*)ws + W.rec_j);
    float* rec_c = (float*)((char*)ws + W.rec_c);
    int32_t* bucket = (int32_t*)((char*)ws + W.bucket);
    double* row_loss = (double*)((char*)ws + W.row_loss);
    int32_t* row_skip = (int32_t*)((char*)ws + W.row_skip);
    int32_t* cnt = (int32_t*)((char*)ws + W.cnt);
    int32_t* first = (int32_t*)((char*)ws + W.first);
    int32_t* cursor = (int32_t*)((char*)ws + W.cursor);
    TripletParams P;
    P.score = spec->score;
    P.loss = spec->loss;
    P.loops = L;
    P.skip_self = spec->self_loops == GNF_TRIPLET_SELF_SKIP;
    P.temp = spec->temp;
    P.shift = spec->shift;
    P.scale = spec->scale_by_sqrt_dim ? 1.f / sqrtf((float)D) : 1.f;
    P.margin = spec->margin;
    P.seed = spec->seed;
    const int words = (max_nodes_per_graph + 63) / 64;   // <= 1024: 12 KiB of LDS
    const size_t lds = (size_t)words * (sizeof(unsigned long long) + sizeof(int32_t));
    hipLaunchKernelGGL(k_triplet_sample, dim3(stats_grid(n)), dim3(64), lds, st, csr->rowptr, csr->col, n, csr->n_edges,
                       csr->node_offsets, b, max_nodes_per_graph, words, z, ld, D, P, draws, rec_j, rec_c, row_loss, row_skip,
                       loss_per_node, pos_index, neg_index);
    GNF_LAUNCH_CHECK("k_triplet_sample");
    hipLaunchKernelGGL(k_triplet_graphs, dim3(stats_grid(b)), dim3(64), 0, st, csr->node_offsets, b, n, max_nodes_per_graph, L,
                       row_loss, row_skip, loss_per_graph, skipped_terms, grad ? 1 : 0, rec_j, rec_c, cnt, first, cursor, bucket);
    GNF_LAUNCH_CHECK("k_triplet_graphs");
    if (grad) {
        const int is_dot = spec->score == GNF_TRIPLET_DOT || spec->score == GNF_TRIPLET_SIGMOID_DOT;
        hipLaunchKernelGGL(k_triplet_grad, dim3(stats_grid(n)), dim3(64), 0, st, z, ld, D, csr->node_offsets, b, n,
                           max_nodes_per_graph, L, is_dot, rec_j, rec_c, cnt, first, bucket, grad, ld_grad, grad_scale);
        GNF_LAUNCH_CHECK("k_triplet_grad");
    }
    hipLaunchKernelGGL(k_triplet_total, dim3(1), dim3(64), 0, st, csr->node_offsets, b, n, max_nodes_per_graph, L,
                       loss_per_graph, skipped_terms, sums2);
    GNF_LAUNCH_CHECK("k_triplet_total");
    return GNF_OK;
}

}  // extern "C"
