// Batch assembly on the device (include/gnf_batches.h): the index arrays of a GraphsTuple and both of its CSRs from a list of
// graph ids into a device-resident dataset (gnf_batch_assemble), or from node counts alone for the complete topology
// (gnf_complete_batch).  Replaces the per-batch host loops of graph_data.py:113-122 and train_grevnet_with_data.py:237-271 and
// the two gnf_build_csr calls behind them; sorts nothing - the dataset-wide CSRs were built once by gnf_build_csr.
//
// Two launches per call:
//   k_batch_scan  one workgroup: per-slot sizes, the exclusive prefix sums over the B slots (node_offsets, and the edge offsets
//                 in ws), the per-slot source offsets.
//   k_batch_fill  ONE launch over every output index array ("jobs": a run of workgroups each).  A thread owns four consecutive
//                 output words at a 16-byte aligned address, finds the owning slot by binary search in the batch's offsets
//                 (LDS copy for B <= GNF_BATCH_LDS_SLOTS, ws beyond) and stores 16 bytes when the four words lie in one graph
//                 and inside the array; group heads / tails and groups across a graph boundary store word by word.
// Every write index is < the job's word count (N + 1 or E, the caller's arguments), every source index is clamped into the
// store's arrays, every slot index into [0, B): data that does not describe the batch gives wrong numbers only.
#include "gnf_common.h"

namespace gnf {

static constexpr int kScanBlock = 1024;
static constexpr int kFillBlock = 256;
static constexpr int kMaxJobs = 6;
static constexpr int kLdsKeys = GNF_BATCH_LDS_SLOTS + 1;

enum FillKind : int32_t {
    kGatherEdges = 0,    // dst[e] = src[src_e0[b] + (e - eb[b])] - src_n0[b] + nb[b]          (senders, receivers, col, col_t)
    kGatherRows = 1,     // dst[i] = src[src_n0[b] + (i - nb[b])] - src_e0[b] + eb[b]          (rowptr, rowptr_t; i = N included)
    kCompleteRows = 2,   // dst[i] = eb[b] + (i - nb[b]) * n_b
    kCompleteSend = 3,   // dst[e] = nb[b] + (e - eb[b]) / n_b
    kCompleteRecv = 4    // dst[e] = nb[b] + (e - eb[b]) % n_b
};

struct FillJob {
    int32_t* dst;
    const int32_t* src;
    int32_t count;   // words of dst
    int32_t kind;
    int32_t shift;   // (address of dst / 4) & 3: group k covers the words [4 k - shift, 4 k - shift + 4)
    int32_t block0;  // first workgroup of the job
    int32_t src_max; // largest valid index of src (-1: src has no words)
    int32_t pad;
};

struct FillArgs {
    FillJob job[kMaxJobs];
    int32_t n_jobs, n_batch;
    int32_t groups_per_thread;
    const int32_t* nb;       // [B + 1] node offsets of the batch (the node_offsets output)
    const int32_t* eb;       // [B + 1] edge offsets of the batch (ws)
    const int64_t* src_e0;   // [B] first edge of slot b's graph in the store (ws; gather kinds only)
    const int32_t* src_n0;   // [B] first node of slot b's graph in the store
};

struct ScanArgs {
    // gnf_batch_assemble: the store's offsets and the ids; gnf_complete_batch: n_node_in
    const int32_t* node_off;
    const int64_t* edge_off;
    const int32_t* graph_ids;
    int64_t n_graphs;
    const int32_t* n_node_in;
    int32_t n_batch;
    int32_t* n_node;   // [B] or NULL (complete)
    int32_t* n_edge;   // [B]
    int32_t* nb;       // [B + 1]
    int32_t* eb;       // [B + 1]
    int64_t* src_e0;   // [B] or NULL
    int32_t* src_n0;   // [B] or NULL
};

__device__ __forceinline__ int32_t clamp_i32(int64_t v) {
    return (int32_t)(v < 0 ? 0 : (v > INT32_MAX ? INT32_MAX : v));
}

template <bool kComplete>
__device__ __forceinline__ void slot_sizes(const ScanArgs& a, int b, int32_t* n, int32_t* e, int64_t* e0, int32_t* n0) {
    if (kComplete) {
        const int32_t v = a.n_node_in[b];
        *n = v < 0 ? 0 : v;
        *e = clamp_i32((int64_t)*n * (int64_t)*n);
        *e0 = 0;
        *n0 = 0;
    } else {
        int64_t g = a.graph_ids[b];
        g = g < 0 ? 0 : (g >= a.n_graphs ? a.n_graphs - 1 : g);   // clamped: wrong numbers, never outside the arrays
        *n0 = a.node_off[g];
        *e0 = a.edge_off[g];
        *n = clamp_i32((int64_t)a.node_off[g + 1] - *n0);
        *e = clamp_i32(a.edge_off[g + 1] - *e0);
    }
}

// one workgroup; thread t owns the slots [t * chunk, (t + 1) * chunk)
template <bool kComplete>
__global__ __launch_bounds__(kScanBlock) void k_batch_scan(ScanArgs a) {
    __shared__ int64_t sn[kScanBlock], se[kScanBlock];
    const int tid = threadIdx.x, B = a.n_batch;
    const int chunk = (B + kScanBlock - 1) / kScanBlock;
    const int beg = tid * chunk < B ? tid * chunk : B, end = beg + chunk < B ? beg + chunk : B;
    int64_t ln = 0, le = 0;
    for (int b = beg; b < end; ++b) {
        int32_t n, e, n0;
        int64_t e0;
        slot_sizes<kComplete>(a, b, &n, &e, &e0, &n0);
        ln += n, le += e;
    }
    sn[tid] = ln, se[tid] = le;
    __syncthreads();
    for (int off = 1; off < kScanBlock; off <<= 1) {   // inclusive scan over the threads' sums
        const int64_t pn = tid >= off ? sn[tid - off] : 0, pe = tid >= off ? se[tid - off] : 0;
        __syncthreads();
        sn[tid] += pn, se[tid] += pe;
        __syncthreads();
    }
    int64_t rn = sn[tid] - ln, re = se[tid] - le;
    for (int b = beg; b < end; ++b) {
        int32_t n, e, n0;
        int64_t e0;
        slot_sizes<kComplete>(a, b, &n, &e, &e0, &n0);
        a.nb[b] = clamp_i32(rn);
        a.eb[b] = clamp_i32(re);
        a.n_edge[b] = e;
        if (!kComplete) {
            a.n_node[b] = n;
            a.src_e0[b] = e0;
            a.src_n0[b] = n0;
        }
        rn += n, re += e;
    }
    if (tid == kScanBlock - 1) {
        a.nb[B] = clamp_i32(sn[tid]);
        a.eb[B] = clamp_i32(se[tid]);
    }
}

// the largest slot b in [0, B) with key[b] <= idx (slot 0 if there is none): the graph that owns word idx - an empty graph
// shares its key with its successor and is passed over; idx past the end lands in the last slot
template <typename Key>
__device__ __forceinline__ int owner_slot(Key key, int B, int32_t idx) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key[mid] <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int32_t fill_value(const FillArgs& a, const FillJob& j, int b, int32_t idx) {
    const int32_t nb = a.nb[b], eb = a.eb[b];
    switch (j.kind) {
        case kGatherEdges: {
            int64_t s = a.src_e0[b] + (int64_t)(idx - eb);
            s = s > j.src_max ? j.src_max : s;
            const int32_t v = s < 0 ? 0 : j.src[s];
            return v - a.src_n0[b] + nb;
        }
        case kGatherRows: {
            int64_t s = (int64_t)a.src_n0[b] + (int64_t)(idx - nb);
            s = s > j.src_max ? j.src_max : s;
            const int32_t v = s < 0 ? 0 : j.src[s];
            return (int32_t)((int64_t)v - a.src_e0[b] + eb);
        }
        case kCompleteRows:
            return (int32_t)((int64_t)eb + (int64_t)(idx - nb) * (int64_t)(a.nb[b + 1] - nb));
        default: {
            int32_t n = a.nb[b + 1] - nb;
            n = n < 1 ? 1 : n;
            const int32_t l = idx - eb, k = l / n;
            return nb + (j.kind == kCompleteSend ? k : l - k * n);
        }
    }
}

template <bool kLds>
__global__ __launch_bounds__(kFillBlock) void k_batch_fill(FillArgs a) {
    __shared__ __attribute__((aligned(16))) int32_t key_sh[kLds ? kLdsKeys : 1];
    const int tid = threadIdx.x, B = a.n_batch;
    int ji = 0;
    for (int q = 1; q < a.n_jobs; ++q)
        if ((int)blockIdx.x >= a.job[q].block0) ji = q;
    const FillJob j = a.job[ji];
    const bool by_node = j.kind == kGatherRows || j.kind == kCompleteRows;
    const int32_t* key_g = by_node ? a.nb : a.eb;   // [B + 1]
    if (kLds) {
        for (int i = tid; i <= B; i += kFillBlock) key_sh[i] = key_g[i];
        __syncthreads();
    }
    const int32_t* key = kLds ? key_sh : key_g;
    const int64_t groups = ((int64_t)j.count + j.shift + 3) >> 2;
    const int64_t g0 = (int64_t)((int)blockIdx.x - j.block0) * kFillBlock * a.groups_per_thread;
    for (int it = 0; it < a.groups_per_thread; ++it) {
        const int64_t grp = g0 + (int64_t)it * kFillBlock + tid;
        if (grp >= groups) break;
        const int64_t first = 4 * grp - j.shift;   // may be negative in group 0 (the head), may run past count in the last
        const int32_t lo = (int32_t)(first < 0 ? 0 : first);
        const int b = owner_slot(key, B, lo);
        if (first >= 0 && first + 4 <= j.count && (b == B - 1 || key[b + 1] > lo + 3)) {
            int4 v;
            v.x = fill_value(a, j, b, lo);
            v.y = fill_value(a, j, b, lo + 1);
            v.z = fill_value(a, j, b, lo + 2);
            v.w = fill_value(a, j, b, lo + 3);
            *reinterpret_cast<int4*>(j.dst + lo) = v;   // 16-byte aligned: (dst / 4 + 4 grp - shift) is a multiple of 4
        } else {
            const int64_t last = first + 4 < j.count ? first + 4 : j.count;
            for (int32_t idx = lo; idx < last; ++idx) j.dst[idx] = fill_value(a, j, owner_slot(key, B, idx), idx);
        }
    }
}

static size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

static int launch_fill(FillArgs& fa, hipStream_t st) {
    int64_t words = 0;
    for (int q = 0; q < fa.n_jobs; ++q) words += fa.job[q].count;
    // large batches: four groups (16 words) per thread - 4096 words per workgroup still leaves > 1400 workgroups at E = 1.45 M;
    // small ones: one group per thread, as many workgroups as there are
    fa.groups_per_thread = words >= (int64_t)1 << 20 ? 4 : 1;
    int64_t blocks = 0;
    for (int q = 0; q < fa.n_jobs; ++q) {
        FillJob& j = fa.job[q];
        j.shift = (int32_t)(((uintptr_t)j.dst >> 2) & 3);
        j.block0 = (int32_t)blocks;
        const int64_t groups = ((int64_t)j.count + j.shift + 3) >> 2;
        const int64_t per = (int64_t)kFillBlock * fa.groups_per_thread;
        blocks += (groups + per - 1) / per;
    }
    if (blocks == 0) return GNF_OK;
    if (fa.n_batch <= GNF_BATCH_LDS_SLOTS)
        hipLaunchKernelGGL(k_batch_fill<true>, dim3((unsigned)blocks), dim3(kFillBlock), 0, st, fa);
    else
        hipLaunchKernelGGL(k_batch_fill<false>, dim3((unsigned)blocks), dim3(kFillBlock), 0, st, fa);
    GNF_LAUNCH_CHECK("k_batch_fill");
    return GNF_OK;
}

static int check_sizes(const char* what, int64_t n_batch, int64_t n_nodes, int64_t n_edges) {
    if (n_batch < 0 || n_nodes < 0 || n_edges < 0 || n_batch > GNF_BATCH_MAX_GRAPHS || n_nodes >= INT32_MAX || n_edges > INT32_MAX) {
        set_error("%s: n_batch=%lld (max %d) n_nodes=%lld n_edges=%lld (int32 rowptr: at most %d)", what, (long long)n_batch,
                  GNF_BATCH_MAX_GRAPHS, (long long)n_nodes, (long long)n_edges, INT32_MAX);
        return GNF_ESHAPE;
    }
    return GNF_OK;
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_batch_assemble_workspace_bytes(int64_t n_batch) {
    if (n_batch < 0 || n_batch > GNF_BATCH_MAX_GRAPHS) return 0;
    // src_e0 int64 [B] | eb int32 [B + 1] | src_n0 int32 [B]
    return align8((size_t)n_batch * 8 + (size_t)(n_batch + 1) * 4 + (size_t)n_batch * 4);
}

int gnf_batch_assemble(const GnfBatchStore* store, const int32_t* graph_ids, int64_t n_batch, int64_t n_nodes, int64_t n_edges,
                       int32_t* n_node, int32_t* n_edge, int32_t* node_offsets, int32_t* senders, int32_t* receivers,
                       int32_t* rowptr, int32_t* col, int32_t* rowptr_t, int32_t* col_t, void* ws, size_t ws_bytes,
                       gnf_stream_t stream) {
    if (!store) {
        set_error("gnf_batch_assemble: null store");
        return GNF_EINVAL;
    }
    if (int rc = check_sizes("gnf_batch_assemble", n_batch, n_nodes, n_edges)) return rc;
    if (store->n_graphs < 0 || store->n_nodes < 0 || store->n_edges < 0 || store->n_nodes >= INT32_MAX || store->n_edges > INT32_MAX ||
        store->n_graphs > INT32_MAX || (store->n_graphs == 0 && n_batch > 0)) {
        set_error("gnf_batch_assemble: store of n_graphs=%lld n_nodes=%lld n_edges=%lld (a batch needs a graph; int32 rowptr)",
                  (long long)store->n_graphs, (long long)store->n_nodes, (long long)store->n_edges);
        return GNF_ESHAPE;
    }
    const bool live = n_batch > 0 && n_nodes > 0;
    if (!rowptr || !rowptr_t || !ws ||
        (live && (!store->node_off || !store->edge_off || !store->rowptr || !store->rowptr_t || !graph_ids || !n_node || !n_edge ||
                  !node_offsets)) ||
        (live && n_edges > 0 && (!senders || !receivers || !col || !col_t)) ||
        (live && n_edges > 0 && store->n_edges > 0 && (!store->senders || !store->receivers || !store->col || !store->col_t))) {
        set_error("gnf_batch_assemble: null pointer argument");
        return GNF_EINVAL;
    }
    if (ws_bytes < gnf_batch_assemble_workspace_bytes(n_batch)) {
        set_error("gnf_batch_assemble: workspace %zu < %zu bytes", ws_bytes, gnf_batch_assemble_workspace_bytes(n_batch));
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!live) {
        GNF_HIP_TRY(hipMemsetAsync(rowptr, 0, sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(rowptr_t, 0, sizeof(int32_t), st));
        return GNF_OK;
    }
    int64_t* src_e0 = (int64_t*)ws;
    int32_t* eb = (int32_t*)(src_e0 + n_batch);
    int32_t* src_n0 = eb + n_batch + 1;
    ScanArgs sa = {};
    sa.node_off = store->node_off, sa.edge_off = store->edge_off, sa.graph_ids = graph_ids, sa.n_graphs = store->n_graphs;
    sa.n_batch = (int32_t)n_batch, sa.n_node = n_node, sa.n_edge = n_edge, sa.nb = node_offsets, sa.eb = eb;
    sa.src_e0 = src_e0, sa.src_n0 = src_n0;
    hipLaunchKernelGGL(k_batch_scan<false>, dim3(1), dim3(kScanBlock), 0, st, sa);
    GNF_LAUNCH_CHECK("k_batch_scan");
    FillArgs fa = {};
    fa.n_batch = (int32_t)n_batch, fa.nb = node_offsets, fa.eb = eb, fa.src_e0 = src_e0, fa.src_n0 = src_n0;
    auto add = [&](int32_t* dst, const int32_t* src, int64_t count, int32_t kind, int64_t src_max) {
        FillJob& j = fa.job[fa.n_jobs++];
        j.dst = dst, j.src = src, j.count = (int32_t)count, j.kind = kind, j.src_max = src ? (int32_t)src_max : -1;
    };
    if (n_edges > 0) {
        add(senders, store->senders, n_edges, kGatherEdges, store->n_edges - 1);
        add(receivers, store->receivers, n_edges, kGatherEdges, store->n_edges - 1);
        add(col, store->col, n_edges, kGatherEdges, store->n_edges - 1);
        add(col_t, store->col_t, n_edges, kGatherEdges, store->n_edges - 1);
    }
    add(rowptr, store->rowptr, n_nodes + 1, kGatherRows, store->n_nodes);
    add(rowptr_t, store->rowptr_t, n_nodes + 1, kGatherRows, store->n_nodes);
    return launch_fill(fa, st);
}

size_t gnf_complete_batch_workspace_bytes(int64_t n_batch) {
    if (n_batch < 0 || n_batch > GNF_BATCH_MAX_GRAPHS) return 0;
    return align8((size_t)(n_batch + 1) * 4);   // eb int32 [B + 1]
}

int gnf_complete_batch(const int32_t* n_node, int64_t n_batch, int64_t n_nodes, int64_t n_edges, int32_t* node_offsets,
                       int32_t* n_edge, int32_t* rowptr, int32_t* senders, int32_t* receivers, void* ws, size_t ws_bytes,
                       gnf_stream_t stream) {
    if (int rc = check_sizes("gnf_complete_batch", n_batch, n_nodes, n_edges)) return rc;
    const bool live = n_batch > 0 && n_nodes > 0;
    if (!rowptr || !ws || (live && (!n_node || !node_offsets || !n_edge)) || (live && n_edges > 0 && (!senders || !receivers))) {
        set_error("gnf_complete_batch: null pointer argument");
        return GNF_EINVAL;
    }
    if (ws_bytes < gnf_complete_batch_workspace_bytes(n_batch)) {
        set_error("gnf_complete_batch: workspace %zu < %zu bytes", ws_bytes, gnf_complete_batch_workspace_bytes(n_batch));
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!live) {
        GNF_HIP_TRY(hipMemsetAsync(rowptr, 0, sizeof(int32_t), st));
        return GNF_OK;
    }
    int32_t* eb = (int32_t*)ws;
    ScanArgs sa = {};
    sa.n_node_in = n_node, sa.n_batch = (int32_t)n_batch, sa.n_edge = n_edge, sa.nb = node_offsets, sa.eb = eb;
    hipLaunchKernelGGL(k_batch_scan<true>, dim3(1), dim3(kScanBlock), 0, st, sa);
    GNF_LAUNCH_CHECK("k_batch_scan");
    FillArgs fa = {};
    fa.n_batch = (int32_t)n_batch, fa.nb = node_offsets, fa.eb = eb;
    auto add = [&](int32_t* dst, int64_t count, int32_t kind) {
        FillJob& j = fa.job[fa.n_jobs++];
        j.dst = dst, j.src = nullptr, j.count = (int32_t)count, j.kind = kind, j.src_max = -1;
    };
    add(rowptr, n_nodes + 1, kCompleteRows);
    if (n_edges > 0) {
        add(senders, n_edges, kCompleteSend);
        add(receivers, n_edges, kCompleteRecv);
    }
    return launch_fill(fa, st);
}

}  // extern "C"
