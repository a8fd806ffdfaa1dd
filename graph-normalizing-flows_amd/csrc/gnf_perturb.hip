// Edge-deletion noise on a batch (include/gnf_perturb.h): the surviving edge list AND both CSRs of the noisy batch from the
// batch's own edge list and CSRs - the producer side of the denoising encoder (run_gnn.py --denoising; graph_data.py:206-280).
// A deletion is a pure function of (seed, min(s, r), max(s, r)), so the three arrays - the edge list, col by receiver, col by
// sender - are compacted independently and still agree on which entries go; gnf_build_csr is stable within a row, so a row's
// survivors in their old order ARE the row gnf_build_csr would make of the filtered list.  No sort, no second builder.
//
// Three launches per call ("array" 0 = the edge list, 1 = the CSR by receiver, 2 = the CSR by sender; W = ceil(E / 64)):
//   k_perturb_mark  one wave per 64 consecutive entries of one array: lane = entry, the pair from (s, r) or from (row of k by
//                   binary search in rowptr, col[k]); the wave's ballot of survivors is the word, written by lane 0.
//   k_perturb_scan  one workgroup: exclusive prefix sums of the words' popcounts per array (base[arr][0 .. W], the last entry
//                   the array's total), of n_edge (segment starts, clamped to [0, E]), and totals.
//   k_perturb_fill  one launch over three regions of workgroups: the entries again (entry k with its bit set goes to
//                   base[k >> 6] + popcount(word & below(k & 63))), the 2 (N + 1) row pointers (that rank at rowptr[i]), the B
//                   graphs (difference of two ranks on the edge list).
// Bounds: a word has bits only for k < E, so a destination is < the array's total <= E; rowptr / n_edge values are clamped
// to [0, E] before they index anything; the row search returns a row in [0, N); node ids only enter the hash.
#include "gnf_common.h"

namespace gnf {

static constexpr int kPerturbBlock = 256;                  // 4 waves = 4 words per workgroup of the mark / fill launches
static constexpr int kPerturbWaves = kPerturbBlock / 64;
static constexpr int kPerturbScanBlock = 1024;

struct PerturbArgs {
    const int32_t *senders, *receivers, *n_edge;
    const int32_t *rowptr, *col, *rowptr_t, *col_t;
    int32_t *senders_out, *receivers_out, *rowptr_out, *col_out, *rowptr_t_out, *col_t_out, *n_edge_out, *num_removed;
    int64_t* totals;
    unsigned long long* words;   // [3][W]
    int32_t* base;               // [3][W + 1]
    int32_t* eb;                 // [B + 1]
    int64_t B, N, E, W;
    uint64_t seed;
    const uint64_t* seed_dev;
    uint64_t threshold;          // deleted iff r32 < threshold (0 .. 2^32)
    int32_t keep_loops;
    int64_t entry_blocks, row_blocks;
};

// the pair's draw of include/gnf_perturb.h
__device__ __forceinline__ uint32_t pair_draw(uint64_t seed, int64_t s, int64_t r) {
    const uint64_t lo = (uint64_t)(s < r ? s : r), hi = (uint64_t)(s < r ? r : s);
    uint64_t x = seed ^ (0x9E3779B97F4A7C15ull * (lo + 1ull)) ^ (0xBF58476D1CE4E5B9ull * (hi + 1ull));
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)(x >> 32);
}

// the largest row i in [0, N) with rowptr[i] <= k (row 0 if there is none): the row that owns entry k - an empty row shares its
// start with its successor and is passed over.  N >= 1.
__device__ __forceinline__ int64_t owner_row(const int32_t* __restrict__ rowptr, int64_t N, int64_t k) {
    int64_t lo = 0, hi = N - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (rowptr[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(kPerturbBlock) void k_perturb_mark(PerturbArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wi = (int64_t)blockIdx.x * kPerturbWaves + (threadIdx.x >> 6);
    if (wi >= 3 * a.W) return;   // the whole wave
    const int arr = (int)(wi / a.W);
    const int64_t w = wi - (int64_t)arr * a.W, k = w * 64 + lane;
    bool keep = false;
    if (k < a.E) {
        int64_t s, r;
        if (arr == 0) {
            s = a.senders[k], r = a.receivers[k];
        } else {
            s = (arr == 1 ? a.col : a.col_t)[k];
            r = owner_row(arr == 1 ? a.rowptr : a.rowptr_t, a.N, k);
        }
        const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
        keep = (s == r && a.keep_loops) || (uint64_t)pair_draw(seed, s, r) >= a.threshold;
    }
    const unsigned long long word = __ballot(keep);
    if (lane == 0) a.words[(int64_t)arr * a.W + w] = word;
}

// one workgroup; thread t owns the words [t * wc, (t + 1) * wc) of each array and the graphs [t * bc, (t + 1) * bc)
__global__ __launch_bounds__(kPerturbScanBlock) void k_perturb_scan(PerturbArgs a) {
    __shared__ int64_t sh[4][kPerturbScanBlock];
    const int tid = threadIdx.x;
    const int64_t W = a.W, B = a.B;
    const int64_t wc = (W + kPerturbScanBlock - 1) / kPerturbScanBlock, bc = (B + kPerturbScanBlock - 1) / kPerturbScanBlock;
    const int64_t wb = tid * wc < W ? tid * wc : W, we = wb + wc < W ? wb + wc : W;
    const int64_t bb = tid * bc < B ? tid * bc : B, be = bb + bc < B ? bb + bc : B;
    int64_t loc[4] = {0, 0, 0, 0};
    for (int64_t w = wb; w < we; ++w)
        for (int q = 0; q < 3; ++q) loc[q] += __popcll(a.words[q * W + w]);
    for (int64_t b = bb; b < be; ++b) {
        const int32_t v = a.n_edge[b];
        loc[3] += v < 0 ? 0 : v;
    }
    for (int q = 0; q < 4; ++q) sh[q][tid] = loc[q];
    __syncthreads();
    for (int off = 1; off < kPerturbScanBlock; off <<= 1) {   // inclusive scan over the threads' sums
        int64_t p[4];
        for (int q = 0; q < 4; ++q) p[q] = tid >= off ? sh[q][tid - off] : 0;
        __syncthreads();
        for (int q = 0; q < 4; ++q) sh[q][tid] += p[q];
        __syncthreads();
    }
    int64_t run[4];
    for (int q = 0; q < 4; ++q) run[q] = sh[q][tid] - loc[q];
    for (int64_t w = wb; w < we; ++w)
        for (int q = 0; q < 3; ++q) {
            a.base[q * (W + 1) + w] = (int32_t)run[q];   // <= E: a word has bits only for entries < E
            run[q] += __popcll(a.words[q * W + w]);
        }
    for (int64_t b = bb; b < be; ++b) {
        const int32_t v = a.n_edge[b];
        a.eb[b] = (int32_t)clamp_to(run[3], a.E);
        run[3] += v < 0 ? 0 : v;
    }
    if (tid == kPerturbScanBlock - 1) {
        for (int q = 0; q < 3; ++q) a.base[q * (W + 1) + W] = (int32_t)sh[q][tid];
        a.eb[B] = (int32_t)clamp_to(sh[3][tid], a.E);
        a.totals[0] = sh[0][tid];
        a.totals[1] = a.E - sh[0][tid];
    }
}

// survivors among the entries [0, p) of array arr, p in [0, E] (so p >> 6 <= W: base has W + 1 entries, the last the total)
__device__ __forceinline__ int32_t rank_at(const PerturbArgs& a, int arr, int64_t p) {
    const int64_t w = p >> 6;
    const int32_t base = a.base[arr * (a.W + 1) + w];
    if (w >= a.W) return base;
    return base + __popcll(a.words[arr * a.W + w] & ((1ull << (p & 63)) - 1ull));
}

__global__ __launch_bounds__(kPerturbBlock) void k_perturb_fill(PerturbArgs a) {
    const int64_t blk = blockIdx.x;
    if (blk < a.entry_blocks) {
        const int lane = threadIdx.x & 63;
        const int64_t wi = blk * kPerturbWaves + (threadIdx.x >> 6);
        if (wi >= 3 * a.W) return;
        const int arr = (int)(wi / a.W);
        const int64_t w = wi - (int64_t)arr * a.W, k = w * 64 + lane;
        const unsigned long long word = a.words[(int64_t)arr * a.W + w];
        if (k >= a.E || !((word >> lane) & 1ull)) return;
        const int64_t dst = (int64_t)a.base[arr * (a.W + 1) + w] + __popcll(word & ((1ull << lane) - 1ull));
        if (dst >= a.E) return;   // cannot happen (dst < the array's total <= E); kept as the bound on the write itself
        if (arr == 0) {
            a.senders_out[dst] = a.senders[k];
            a.receivers_out[dst] = a.receivers[k];
        } else if (arr == 1) {
            a.col_out[dst] = a.col[k];
        } else {
            a.col_t_out[dst] = a.col_t[k];
        }
    } else if (blk < a.entry_blocks + a.row_blocks) {
        const int64_t idx = (blk - a.entry_blocks) * kPerturbBlock + threadIdx.x;
        if (idx >= 2 * (a.N + 1)) return;
        const int t = idx > a.N;
        const int64_t i = idx - t * (a.N + 1);
        const int64_t p = clamp_to((t ? a.rowptr_t : a.rowptr)[i], a.E);
        (t ? a.rowptr_t_out : a.rowptr_out)[i] = rank_at(a, 1 + t, p);
    } else {
        const int64_t b = (blk - a.entry_blocks - a.row_blocks) * kPerturbBlock + threadIdx.x;
        if (b >= a.B) return;
        const int64_t lo = a.eb[b], hi = a.eb[b + 1];   // clamped to [0, E] and ascending by k_perturb_scan
        const int32_t kept = rank_at(a, 0, hi) - rank_at(a, 0, lo);
        a.n_edge_out[b] = kept;
        a.num_removed[b] = (int32_t)(hi - lo) - kept;
    }
}

static size_t perturb_align8(size_t v) { return (v + 7) & ~(size_t)7; }

static bool perturb_sizes_ok(int64_t b, int64_t n, int64_t e) {
    return b >= 0 && n >= 0 && e >= 0 && b <= INT32_MAX && n <= INT32_MAX && e <= INT32_MAX;
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_perturb_edges_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int64_t n_edges) {
    if (!perturb_sizes_ok(n_graphs, n_nodes, n_edges)) return 0;
    const size_t W = ((size_t)n_edges + 63) / 64;
    // words uint64 [3][W] | base int32 [3][W + 1] | eb int32 [B + 1]
    return perturb_align8(3 * W * 8 + 3 * (W + 1) * 4 + ((size_t)n_graphs + 1) * 4);
}

int gnf_perturb_edges(const int32_t* senders, const int32_t* receivers, const int32_t* n_edge, const GnfCsr* csr,
                      const GnfCsr* csr_t, const GnfPerturbSpec* spec, int32_t* senders_out, int32_t* receivers_out,
                      int32_t* rowptr_out, int32_t* col_out, int32_t* rowptr_t_out, int32_t* col_t_out, int32_t* n_edge_out,
                      int32_t* num_removed, int64_t* totals, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    if (!csr || !csr_t || !spec) {
        set_error("gnf_perturb_edges: null csr / csr_t / spec");
        return GNF_EINVAL;
    }
    const int64_t B = csr->n_graphs, N = csr->n_nodes, E = csr->n_edges;
    if (!perturb_sizes_ok(B, N, E) || csr_t->n_graphs != B || csr_t->n_nodes != N || csr_t->n_edges != E) {
        set_error("gnf_perturb_edges: csr of n_graphs=%lld n_nodes=%lld n_edges=%lld, csr_t of %lld / %lld / %lld (equal, >= 0, "
                  "at most %d: int32 rowptr)", (long long)B, (long long)N, (long long)E, (long long)csr_t->n_graphs,
                  (long long)csr_t->n_nodes, (long long)csr_t->n_edges, INT32_MAX);
        return GNF_ESHAPE;
    }
    const bool live = B > 0 && N > 0;
    if (!rowptr_out || !rowptr_t_out || !totals || !ws) {
        set_error("gnf_perturb_edges: null pointer argument (rowptr_out / rowptr_t_out / totals / ws)");
        return GNF_EINVAL;
    }
    if (live && (!csr->node_offsets || !csr_t->node_offsets)) {
        set_error("gnf_perturb_edges: csr->node_offsets and csr_t->node_offsets are required");
        return GNF_EINVAL;
    }
    if ((live && (!n_edge || !csr->rowptr || !csr_t->rowptr || !n_edge_out || !num_removed)) ||
        (live && E > 0 && (!senders || !receivers || !csr->col || !csr_t->col || !senders_out || !receivers_out || !col_out ||
                           !col_t_out))) {
        set_error("gnf_perturb_edges: null pointer argument");
        return GNF_EINVAL;
    }
    if (spec->self_loops != GNF_PERTURB_LOOPS_KEEP && spec->self_loops != GNF_PERTURB_LOOPS_DRAW) {
        set_error("gnf_perturb_edges: self_loops=%d", (int)spec->self_loops);
        return GNF_EINVAL;
    }
    if (!(spec->deletion_prob >= 0.0 && spec->deletion_prob <= 1.0)) {
        set_error("gnf_perturb_edges: deletion_prob=%g is not in [0, 1]", spec->deletion_prob);
        return GNF_EINVAL;
    }
    const size_t need = gnf_perturb_edges_workspace_bytes(B, N, E);
    if (ws_bytes < need) {
        set_error("gnf_perturb_edges: workspace %zu < %zu bytes", ws_bytes, need);
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!live) {
        GNF_HIP_TRY(hipMemsetAsync(rowptr_out, 0, sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(rowptr_t_out, 0, sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
        return GNF_OK;
    }
    PerturbArgs a = {};
    a.senders = senders, a.receivers = receivers, a.n_edge = n_edge;
    a.rowptr = csr->rowptr, a.col = csr->col, a.rowptr_t = csr_t->rowptr, a.col_t = csr_t->col;
    a.senders_out = senders_out, a.receivers_out = receivers_out, a.rowptr_out = rowptr_out, a.col_out = col_out;
    a.rowptr_t_out = rowptr_t_out, a.col_t_out = col_t_out, a.n_edge_out = n_edge_out, a.num_removed = num_removed;
    a.totals = totals;
    a.B = B, a.N = N, a.E = E, a.W = (E + 63) / 64;
    a.words = (unsigned long long*)ws;
    a.base = (int32_t*)(a.words + 3 * a.W);
    a.eb = a.base + 3 * (a.W + 1);
    a.seed = spec->seed, a.seed_dev = spec->seed_dev;
    a.threshold = (uint64_t)(spec->deletion_prob * 4294967296.0);
    a.keep_loops = spec->self_loops == GNF_PERTURB_LOOPS_KEEP;
    a.entry_blocks = (3 * a.W + kPerturbWaves - 1) / kPerturbWaves;
    a.row_blocks = (2 * (N + 1) + kPerturbBlock - 1) / kPerturbBlock;
    const int64_t graph_blocks = (B + kPerturbBlock - 1) / kPerturbBlock;
    if (a.entry_blocks > 0) {
        hipLaunchKernelGGL(k_perturb_mark, dim3((unsigned)a.entry_blocks), dim3(kPerturbBlock), 0, st, a);
        GNF_LAUNCH_CHECK("k_perturb_mark");
    }
    hipLaunchKernelGGL(k_perturb_scan, dim3(1), dim3(kPerturbScanBlock), 0, st, a);
    GNF_LAUNCH_CHECK("k_perturb_scan");
    hipLaunchKernelGGL(k_perturb_fill, dim3((unsigned)(a.entry_blocks + a.row_blocks + graph_blocks)), dim3(kPerturbBlock), 0, st, a);
    GNF_LAUNCH_CHECK("k_perturb_fill");
    return GNF_OK;
}

}  // extern "C"
