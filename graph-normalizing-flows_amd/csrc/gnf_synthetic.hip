// The GRevNet driver's synthetic datasets as ready batches on the device (include/gnf_synthetic.h): the complete topology with
// self loops in the order of fully_connected_edge_list with both of its CSRs (gnf_synthetic_topology), and the node features of
// two moons / mixtures of Gaussians from a defined integer hash (gnf_synthetic_nodes).  Replaces the per-iteration host loop
// of grevnet_synthetic_data.py:17-21, 28-47, 50-79, the upload and the two gnf_build_csr calls behind it.
//
// gnf_synthetic_topology, two launches:
//   k_syn_scan   one workgroup: counts clamped at 0, the exclusive prefix sums over the B graphs (node_offsets, and the edge
//                offsets in ws), n_edge.
//   k_syn_fill   ONE launch over rowptr, senders, receivers and col ("jobs": a run of workgroups each).  A thread owns four
//                consecutive output words at a 16-byte aligned address, finds the owning graph by binary search in the offsets
//                and stores 16 bytes when the four words lie in one graph and inside the array; heads, tails and groups across
//                a graph boundary store word by word.  The offsets are read from global memory: at the drivers' B = 32 the
//                search is five loads of one cache line.
// gnf_synthetic_nodes, one launch:
//   k_syn_nodes  thread = node index t: graph b by binary search, template index i = t - node_offsets[b]; rank(i) by
//                recomputing the graph's n keys (two hash rounds each: the first round is the graph's and hoisted), the point,
//                the Gaussian pair of node rank(i), the write of row node_offsets[b] + rank(i).
// Bounds: every write index is < the job's word count (N + 1 or E) or < N (the caller's arguments); graph indices are in
// [0, B); the offsets table of a mog spec is read at set * set_stride + i with set in [0, n_sets) and i < set_size <= set_stride.
#include <math.h>

#include "gnf_common.h"

namespace gnf {

static constexpr int kSynScanBlock = 1024;
static constexpr int kSynBlock = 256;
static constexpr int kSynJobs = 4;

enum SynKind : int32_t {
    kSynRows = 0,   // rowptr[i]    = eb[b] + (i - nb[b]) * n_b                       (i = N included)
    kSynSend = 1,   // senders[e]   = nb[b] + k,  k = (e - eb[b]) / n_b
    kSynRecv = 2,   // receivers[e] = nb[b] + (p == n_b - 1 ? k : p + (p >= k)),  p = (e - eb[b]) % n_b
    kSynCol = 3     // col[e]       = nb[b] + p
};

struct SynJob {
    int32_t* dst;
    int32_t count;   // words of dst
    int32_t kind;
    int32_t shift;   // (address of dst / 4) & 3: group k covers the words [4 k - shift, 4 k - shift + 4)
    int32_t block0;  // first workgroup of the job
};

struct SynFillArgs {
    SynJob job[kSynJobs];
    int32_t n_jobs, n_batch;
    const int32_t* nb;   // [B + 1] node offsets (the node_offsets output)
    const int32_t* eb;   // [B + 1] edge offsets (ws)
};

struct SynScanArgs {
    const int32_t* n_node;
    int32_t n_batch;
    int32_t* n_edge;   // [B]
    int32_t* nb;       // [B + 1]
    int32_t* eb;       // [B + 1]
};

__device__ __forceinline__ int32_t syn_clamp_i32(int64_t v) { return (int32_t)(v < 0 ? 0 : (v > INT32_MAX ? INT32_MAX : v)); }

// one workgroup; thread t owns the graphs [t * chunk, (t + 1) * chunk)
__global__ __launch_bounds__(kSynScanBlock) void k_syn_scan(SynScanArgs a) {
    __shared__ int64_t sn[kSynScanBlock], se[kSynScanBlock];
    const int tid = threadIdx.x, B = a.n_batch;
    const int chunk = (B + kSynScanBlock - 1) / kSynScanBlock;
    const int beg = tid * chunk < B ? tid * chunk : B, end = beg + chunk < B ? beg + chunk : B;
    int64_t ln = 0, le = 0;
    for (int b = beg; b < end; ++b) {
        const int64_t n = a.n_node[b] < 0 ? 0 : a.n_node[b];
        ln += n, le += n * n;
    }
    sn[tid] = ln, se[tid] = le;
    __syncthreads();
    for (int off = 1; off < kSynScanBlock; off <<= 1) {   // inclusive scan over the threads' sums
        const int64_t pn = tid >= off ? sn[tid - off] : 0, pe = tid >= off ? se[tid - off] : 0;
        __syncthreads();
        sn[tid] += pn, se[tid] += pe;
        __syncthreads();
    }
    int64_t rn = sn[tid] - ln, re = se[tid] - le;
    for (int b = beg; b < end; ++b) {
        const int64_t n = a.n_node[b] < 0 ? 0 : a.n_node[b];
        a.nb[b] = syn_clamp_i32(rn);
        a.eb[b] = syn_clamp_i32(re);
        a.n_edge[b] = syn_clamp_i32(n * n);
        rn += n, re += n * n;
    }
    if (tid == kSynScanBlock - 1) {
        a.nb[B] = syn_clamp_i32(sn[tid]);
        a.eb[B] = syn_clamp_i32(se[tid]);
    }
}

// the largest graph b in [0, B) with key[b] <= idx (graph 0 if there is none): the graph that owns word idx - an empty graph
// shares its key with its successor and is passed over; idx past the end lands in the last graph.  B >= 1.
__device__ __forceinline__ int syn_owner(const int32_t* __restrict__ key, int B, int32_t idx) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key[mid] <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int32_t syn_fill_value(const SynFillArgs& a, int kind, int b, int32_t idx) {
    const int32_t nb = a.nb[b], eb = a.eb[b], n_raw = a.nb[b + 1] - nb;
    if (kind == kSynRows) return (int32_t)((int64_t)eb + (int64_t)(idx - nb) * (int64_t)n_raw);
    const int32_t n = n_raw < 1 ? 1 : n_raw;
    const int32_t l = idx - eb, k = l / n, p = l - k * n;
    if (kind == kSynSend) return nb + k;
    if (kind == kSynCol) return nb + p;
    return nb + (p == n - 1 ? k : p + (p >= k ? 1 : 0));
}

__global__ __launch_bounds__(kSynBlock) void k_syn_fill(SynFillArgs a) {
    const int tid = threadIdx.x, B = a.n_batch;
    int ji = 0;
    for (int q = 1; q < a.n_jobs; ++q)
        if ((int)blockIdx.x >= a.job[q].block0) ji = q;
    const SynJob j = a.job[ji];
    const int32_t* key = j.kind == kSynRows ? a.nb : a.eb;   // [B + 1]
    const int64_t groups = ((int64_t)j.count + j.shift + 3) >> 2;
    const int64_t grp = (int64_t)((int)blockIdx.x - j.block0) * kSynBlock + tid;
    if (grp >= groups) return;
    const int64_t first = 4 * grp - j.shift;   // may be negative in group 0 (the head), may run past count in the last
    const int32_t lo = (int32_t)(first < 0 ? 0 : first);
    const int b = syn_owner(key, B, lo);
    if (first >= 0 && first + 4 <= j.count && (b == B - 1 || key[b + 1] > lo + 3)) {
        int4 v;
        v.x = syn_fill_value(a, j.kind, b, lo);
        v.y = syn_fill_value(a, j.kind, b, lo + 1);
        v.z = syn_fill_value(a, j.kind, b, lo + 2);
        v.w = syn_fill_value(a, j.kind, b, lo + 3);
        *reinterpret_cast<int4*>(j.dst + lo) = v;   // 16-byte aligned: (dst / 4 + 4 grp - shift) is a multiple of 4
    } else {
        const int64_t last = first + 4 < j.count ? first + 4 : j.count;
        for (int32_t idx = lo; idx < last; ++idx) j.dst[idx] = syn_fill_value(a, j.kind, syn_owner(key, B, idx), idx);
    }
}

struct SynNodeArgs {
    uint64_t seed;
    const uint64_t* seed_dev;
    const int32_t *n_node, *set_id, *node_offsets;
    const float* offsets;
    float* nodes;
    int32_t* source;
    int64_t ld;
    int32_t n_batch, n_nodes, max_n;
    int32_t kind, rotate, n_sets, set_stride;
    int32_t set_size[GNF_SYN_MAX_SETS];
    float noise;
};

static constexpr float kSynPi = 3.14159265358979f, kSynTwoPi = 6.28318530717959f, kSynInv24 = 1.0f / 16777216.0f;

__global__ __launch_bounds__(kSynBlock) void k_syn_nodes(SynNodeArgs a) {
    const int64_t t64 = (int64_t)blockIdx.x * kSynBlock + threadIdx.x;
    if (t64 >= a.n_nodes) return;
    const int32_t t = (int32_t)t64;
    const int b = syn_owner(a.node_offsets, a.n_batch, t);
    const int32_t o = a.node_offsets[b], i = t - o;
    int32_t n = a.n_node[b];
    n = n < 0 ? 0 : (n > a.max_n ? a.max_n : n);
    if (i < 0 || i >= n) return;   // offsets that do not describe the batch: this thread has no template point
    const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
    // gnf_syn_draw(seed, b, q, stream) with its first round, the graph's, done once
    const uint64_t gx = gnf_syn_mix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)b + 1ull));
    auto draw = [gx](uint32_t index, uint32_t stream) {
        const uint64_t x = gnf_syn_mix64(gx ^ (0xBF58476D1CE4E5B9ull * ((uint64_t)index + 1ull)));
        return (uint32_t)(gnf_syn_mix64(x ^ (0x94D049BB133111EBull * ((uint64_t)stream + 1ull))) >> 32);
    };
    const uint32_t mine = draw((uint32_t)i, GNF_SYN_STREAM_KEY);
    int32_t rank = 0;
    for (int32_t q = 0; q < n; ++q) {
        const uint32_t kq = draw((uint32_t)q, GNF_SYN_STREAM_KEY);
        rank += (kq < mine || (kq == mine && q < i)) ? 1 : 0;
    }
    const int64_t row = (int64_t)o + rank;
    if (row < 0 || row >= a.n_nodes) return;   // cannot happen for offsets that describe the batch; the bound on the write
    // the Gaussian pair of node `rank`
    const float u1 = (float)((draw((uint32_t)rank, GNF_SYN_STREAM_U1) >> 8) + 1u) * kSynInv24;
    const float u2 = (float)(draw((uint32_t)rank, GNF_SYN_STREAM_U2) >> 8) * kSynInv24;
    const float r = sqrtf(-2.0f * logf(u1)), ang = kSynTwoPi * u2;
    const float z0 = r * cosf(ang), z1 = r * sinf(ang);
    float x, y;
    if (a.kind == GNF_SYN_MOONS) {
        const int32_t n_out = n / 2, n_in = n - n_out;
        if (i < n_out) {
            const float th = n_out > 1 ? (float)i * (kSynPi / (float)(n_out - 1)) : 0.0f;
            x = cosf(th), y = sinf(th);
        } else {
            const float th = n_in > 1 ? (float)(i - n_out) * (kSynPi / (float)(n_in - 1)) : 0.0f;
            x = 1.0f - cosf(th), y = 0.5f - sinf(th);
        }
        if (a.noise != 0.0f) x += a.noise * z0, y += a.noise * z1;
    } else {
        int32_t set = a.set_id ? a.set_id[b] : 0;
        set = set < 0 ? 0 : (set >= a.n_sets ? a.n_sets - 1 : set);
        int32_t size = 0;   // a select per entry: a lane-varying index into the kernel arguments would go through scratch
        for (int q = 0; q < GNF_SYN_MAX_SETS; ++q) size = q == set ? a.set_size[q] : size;
        float ox = 0.0f, oy = 0.0f;
        if (i < size) {
            const float* p = a.offsets + 2 * ((int64_t)set * a.set_stride + i);
            ox = p[0], oy = p[1];
        }
        x = z0 + ox, y = z1 + oy;
        if (a.rotate) {
            const float al = (float)(draw(0u, GNF_SYN_STREAM_ANGLE) >> 8) * kSynInv24 * kSynPi;
            const float c = cosf(al), s = sinf(al);
            const float xr = x * c - y * s, yr = x * s + y * c;
            x = xr, y = yr;
        }
    }
    float* out = a.nodes + row * a.ld;
    out[0] = x, out[1] = y;
    if (a.source) a.source[row] = i;
}

static size_t syn_align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_synthetic_topology_workspace_bytes(int64_t n_batch) {
    if (n_batch < 0 || n_batch > GNF_BATCH_MAX_GRAPHS) return 0;
    return syn_align8((size_t)(n_batch + 1) * 4);   // eb int32 [B + 1]
}

int gnf_synthetic_topology(const int32_t* n_node, int64_t n_batch, int64_t n_nodes, int64_t n_edges, int32_t* node_offsets,
                           int32_t* n_edge, int32_t* rowptr, int32_t* senders, int32_t* receivers, int32_t* col, void* ws,
                           size_t ws_bytes, gnf_stream_t stream) {
    if (n_batch < 0 || n_nodes < 0 || n_edges < 0 || n_batch > GNF_BATCH_MAX_GRAPHS || n_nodes >= INT32_MAX || n_edges > INT32_MAX) {
        set_error("gnf_synthetic_topology: n_batch=%lld (max %d) n_nodes=%lld n_edges=%lld (int32 rowptr: at most %d)",
                  (long long)n_batch, GNF_BATCH_MAX_GRAPHS, (long long)n_nodes, (long long)n_edges, INT32_MAX);
        return GNF_ESHAPE;
    }
    const bool live = n_batch > 0 && n_nodes > 0;
    if (!rowptr || !ws || (live && (!n_node || !node_offsets || !n_edge)) ||
        (live && n_edges > 0 && (!senders || !receivers || !col))) {
        set_error("gnf_synthetic_topology: null pointer argument");
        return GNF_EINVAL;
    }
    if (ws_bytes < gnf_synthetic_topology_workspace_bytes(n_batch)) {
        set_error("gnf_synthetic_topology: workspace %zu < %zu bytes", ws_bytes, gnf_synthetic_topology_workspace_bytes(n_batch));
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!live) {
        GNF_HIP_TRY(hipMemsetAsync(rowptr, 0, sizeof(int32_t), st));
        return GNF_OK;
    }
    int32_t* eb = (int32_t*)ws;
    SynScanArgs sa = {};
    sa.n_node = n_node, sa.n_batch = (int32_t)n_batch, sa.n_edge = n_edge, sa.nb = node_offsets, sa.eb = eb;
    hipLaunchKernelGGL(k_syn_scan, dim3(1), dim3(kSynScanBlock), 0, st, sa);
    GNF_LAUNCH_CHECK("k_syn_scan");
    SynFillArgs fa = {};
    fa.n_batch = (int32_t)n_batch, fa.nb = node_offsets, fa.eb = eb;
    int64_t blocks = 0;
    auto add = [&](int32_t* dst, int64_t count, int32_t kind) {
        SynJob& j = fa.job[fa.n_jobs++];
        j.dst = dst, j.count = (int32_t)count, j.kind = kind;
        j.shift = (int32_t)(((uintptr_t)dst >> 2) & 3);
        j.block0 = (int32_t)blocks;
        const int64_t groups = (count + j.shift + 3) >> 2;
        blocks += (groups + kSynBlock - 1) / kSynBlock;
    };
    add(rowptr, n_nodes + 1, kSynRows);
    if (n_edges > 0) {
        add(senders, n_edges, kSynSend);
        add(receivers, n_edges, kSynRecv);
        add(col, n_edges, kSynCol);
    }
    hipLaunchKernelGGL(k_syn_fill, dim3((unsigned)blocks), dim3(kSynBlock), 0, st, fa);
    GNF_LAUNCH_CHECK("k_syn_fill");
    return GNF_OK;
}

int gnf_synthetic_nodes(const GnfSyntheticSpec* spec, const int32_t* n_node, const int32_t* set_id, const int32_t* node_offsets,
                        int64_t n_batch, int64_t n_nodes, int32_t max_nodes_per_graph, float* nodes, int64_t ld, int32_t* source,
                        gnf_stream_t stream) {
    if (!spec) {
        set_error("gnf_synthetic_nodes: null spec");
        return GNF_EINVAL;
    }
    if (n_batch < 0 || n_nodes < 0 || n_batch > GNF_BATCH_MAX_GRAPHS || n_nodes >= INT32_MAX || ld < 2 || max_nodes_per_graph < 1 ||
        max_nodes_per_graph > GNF_SYN_MAX_NODES) {
        set_error("gnf_synthetic_nodes: n_batch=%lld (max %d) n_nodes=%lld (below %d) ld=%lld (>= 2) max_nodes_per_graph=%d "
                  "(1 .. %d)", (long long)n_batch, GNF_BATCH_MAX_GRAPHS, (long long)n_nodes, INT32_MAX, (long long)ld,
                  (int)max_nodes_per_graph, GNF_SYN_MAX_NODES);
        return GNF_ESHAPE;
    }
    if (spec->kind != GNF_SYN_MOONS && spec->kind != GNF_SYN_MOG) {
        set_error("gnf_synthetic_nodes: kind=%d", (int)spec->kind);
        return GNF_EINVAL;
    }
    if (spec->kind == GNF_SYN_MOONS && !(spec->noise >= 0.0)) {
        set_error("gnf_synthetic_nodes: noise=%g is negative or NaN", spec->noise);
        return GNF_EINVAL;
    }
    if (spec->kind == GNF_SYN_MOG) {
        bool ok = spec->offsets && spec->n_sets >= 1 && spec->n_sets <= GNF_SYN_MAX_SETS && spec->set_stride >= 0;
        for (int q = 0; ok && q < spec->n_sets; ++q) ok = spec->set_size[q] >= 0 && spec->set_size[q] <= spec->set_stride;
        if (!ok) {
            set_error("gnf_synthetic_nodes: a mixture needs offsets, n_sets=%d in 1 .. %d and every set_size in 0 .. "
                      "set_stride=%d", (int)spec->n_sets, GNF_SYN_MAX_SETS, (int)spec->set_stride);
            return GNF_EINVAL;
        }
    }
    const bool live = n_batch > 0 && n_nodes > 0;
    if (live && (!n_node || !node_offsets || !nodes)) {
        set_error("gnf_synthetic_nodes: null pointer argument (n_node / node_offsets / nodes)");
        return GNF_EINVAL;
    }
    if (!live) return GNF_OK;
    SynNodeArgs a = {};
    a.seed = spec->seed, a.seed_dev = spec->seed_dev;
    a.n_node = n_node, a.set_id = set_id, a.node_offsets = node_offsets, a.offsets = spec->offsets;
    a.nodes = nodes, a.source = source, a.ld = ld;
    a.n_batch = (int32_t)n_batch, a.n_nodes = (int32_t)n_nodes, a.max_n = max_nodes_per_graph;
    a.kind = spec->kind, a.rotate = spec->rotate != 0;
    if (spec->kind == GNF_SYN_MOG) {
        a.n_sets = spec->n_sets, a.set_stride = spec->set_stride;
        for (int q = 0; q < spec->n_sets; ++q) a.set_size[q] = spec->set_size[q];
    }
    a.noise = spec->kind == GNF_SYN_MOONS ? (float)spec->noise : 0.0f;
    const int64_t blocks = (n_nodes + kSynBlock - 1) / kSynBlock;
    hipLaunchKernelGGL(k_syn_nodes, dim3((unsigned)blocks), dim3(kSynBlock), 0, (hipStream_t)stream, a);
    GNF_LAUNCH_CHECK("k_syn_nodes");
    return GNF_OK;
}

}  // extern "C"
