// Weisfeiler-Lehman hashes of every graph of a batch and the matching of two hash sets - uniqueness and novelty of generated
// graphs, the figure of the GraphRNN / GRAN tables that the four MMDs (gnf_graph_stats / _orbits / _spectra) cannot see: a
// sampler that replays its training set scores a perfect MMD.  The reference stops at pickling the graphs
// (generate_graphs.py:68-84); nothing in it corresponds to these kernels.
//
// Graph model and bitmap: as in gnf_graph_stats.hip (undirected, simple), built by build_graph_bitmap (gnf_graph_bitmap.h:
// k_stats_bitmap on a zeroed bitmap).  The hash is DEFINED in include/gnf_graph_hashes.h (wl_mix and the four constants below restate it): every
// sum in it is a wrapping 64-bit integer sum, so neither the order of the nodes nor the order in which lanes, waves or atomics
// add changes a bit, and the two routes below agree bit for bit.
//
// gnf_graph_hashes.  k_stats_bitmap, then, chosen on the host from max_nodes_per_graph:
//   LDS route (<= GNF_WL_LDS_NODES = 4096): k_wl_lds, one workgroup per graph striding over graphs, 256 threads up to 256
//     columns and 1024 above.  LDS: cur [cap] | nxt [cap] 64-bit colours (dynamic, 16 cap bytes <= 64 KiB) and 2 x 2 x 16 wave
//     slots (static): two workgroups fit a CU's 160 KiB, and two of 1024 threads are its 32 waves.  A wave per node row: the
//     lanes take the row's words, walk their set bits and add mix(cur[j] ^ KB) from LDS (rows of at most 256 columns: a lane per
//     column instead, wl_neighbour_sum), then a wave sum; lane 0 writes nxt[i].
//     Every wave keeps its running sum_i mix(c'_i ^ KA) in a register and leaves it in its slot; after the round's ONE barrier
//     every thread adds the slots in wave order and updates h alike.  The slots alternate with the round's parity, as the
//     colour arrays do: a wave can only write round t + 1's slots and colours after every wave has passed round t's barrier,
//     i.e. has read what round t - 1 left there.
//   global route (above): k_wl_init / k_wl_round, a wave per node, grid-stride; colours in two workspace arrays (the last
//     round writes node_colour itself), per-graph sums by 64-bit atomicAdd into a zeroed table [iterations + 1][B], degree sums
//     into n_edges; k_wl_fold, a thread per graph, halves the degree sum and folds the table into h in round order.
// Loop bounds (binding): rows i < n_g, words w < ceil(n_g / 64), at most 64 set bits per word (the last word is masked to the
// graph's columns, so a colour index never leaves [0, n_g)), rounds t <= iterations - whatever the bitmap holds.
// Cost per graph: the bitmap is read iterations + 1 times, n_g W 8 bytes each; one mix per directed edge and round.
//
// gnf_graph_hash_match.  k_hash_match, a wave per graph g of A: the lanes stride over A[0 .. g) and over B comparing (hash,
// n_node), a wave minimum each, and lane 0 adds to the four counts with integer atomics.
#include "gnf_graph_bitmap.h"

namespace gnf {

static constexpr int kWlMaxNodes = GNF_WL_MAX_NODES, kWlLdsNodes = GNF_WL_LDS_NODES, kWlMaxIter = GNF_WL_MAX_ITERATIONS;
static constexpr int kWlMaxWaves = 16;   // of a k_wl_lds workgroup
static constexpr int kWlColumnWords = 4;   // rows up to 256 columns: a lane per column, see wl_neighbour_sum
static constexpr unsigned long long kWlA = 0xA5A5A5A5A5A5A5A5ull, kWlB = 0xD6E8FEB86659FD93ull, kWlC = 0xFF51AFD7ED558CCDull,
                                    kWlD = 0xC4CEB9FE1A85EC53ull, kWlSize = 0x100000001B3ull;

__device__ __forceinline__ unsigned long long wl_mix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// caller-owned workspace of gnf_graph_hashes (host only): the gnf_graph_stats workspace (bitmap, gid) | colour buffers uint64 [N]
// x 2 | table uint64 [kWlMaxIter + 1][B].  One layout for both routes; the LDS route uses the bitmap alone.
struct WlWs {
    StatsWs stats;
    size_t col_a, col_b, table, total;
};
static WlWs wl_ws(int64_t n_graphs, int64_t n_nodes, int32_t cap) {
    WlWs L;
    L.stats = stats_ws(n_nodes, cap);
    L.col_a = L.stats.total;
    L.col_b = L.col_a + (size_t)n_nodes * sizeof(uint64_t);
    L.table = L.col_b + (size_t)n_nodes * sizeof(uint64_t);
    L.total = L.table + (size_t)(kWlMaxIter + 1) * (size_t)n_graphs * sizeof(uint64_t);
    return L;
}

// the bits of word w of a row that are columns of the graph (n columns): the colour index w * 64 + bit stays below n
__device__ __forceinline__ unsigned long long wl_row_word(const unsigned long long* __restrict__ row, int w, int n) {
    const int tail = n - w * 64;
    const unsigned long long bits = row[w];
    return tail >= 64 ? bits : bits & ((1ull << tail) - 1ull);
}

// sum_{j in N(i)} mix(colour[j] ^ KB) of one row, by one wave (every lane gets the sum).  A row of at most kWlColumnWords words is
// read with a lane per COLUMN, word after word - on a small or dense graph every lane has work; a longer row with a lane per
// WORD that walks its set bits - a sparse row of many words costs a few steps.  The same terms either way, and the sum wraps:
// the same bits.
__device__ __forceinline__ unsigned long long wl_neighbour_sum(const unsigned long long* __restrict__ row, int words, int n,
                                                               const unsigned long long* colour, int lane) {
    unsigned long long sum = 0ull;
    if (words <= kWlColumnWords) {   // (uniform over the wave)
        for (int w = 0; w < words; ++w)
            if ((wl_row_word(row, w, n) >> lane) & 1ull) sum += wl_mix(colour[w * 64 + lane] ^ kWlB);
    } else {
        for (int w = lane; w < words; w += 64)
            for (unsigned long long bits = wl_row_word(row, w, n); bits; bits &= bits - 1ull)
                sum += wl_mix(colour[w * 64 + __ffsll((long long)bits) - 1] ^ kWlB);
    }
    return wave_sum_u64(sum);
}

// ---- LDS route -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_wl_lds(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes, int cap,
                                                 int64_t W, const unsigned long long* __restrict__ bitmap,
                                                 const int64_t* __restrict__ labels, int iterations,
                                                 unsigned long long* __restrict__ hash,
                                                 unsigned long long* __restrict__ node_colour, int64_t* __restrict__ n_edges) {
    extern __shared__ unsigned long long wl_lds[];                 // cur [cap] | nxt [cap]
    __shared__ unsigned long long slot[2][2][kWlMaxWaves];         // [round parity][colour sum, degree sum][wave]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;

    for (int64_t g = blockIdx.x; g < n_graphs; g += gridDim.x) {   // (uniform over the workgroup)
        int64_t n0;
        int n;
        stats_graph_range(off, (int)g, n_nodes, cap, n0, n);
        const int words = (n + 63) / 64;
        unsigned long long* cur = wl_lds;
        unsigned long long* nxt = wl_lds + cap;
        __syncthreads();   // the previous graph's readers of the colours and slots are done
        // initial colours: the degree of the row, or the caller's label
        unsigned long long acc = 0ull, deg = 0ull;   // (the same in every lane of a wave)
        for (int i = wave; i < n; i += waves) {
            const unsigned long long* row = bitmap + (n0 + i) * W;
            unsigned long long d = 0ull;
            for (int w = lane; w < words; w += 64) d += __popcll(wl_row_word(row, w, n));
            d = wave_sum_u64(d);
            const unsigned long long c = wl_mix(labels ? (unsigned long long)labels[n0 + i] : d);
            if (lane == 0) cur[i] = c;
            acc += wl_mix(c ^ kWlA);
            deg += d;
        }
        if (lane == 0) {
            slot[0][0][wave] = acc;
            slot[0][1][wave] = deg;
        }
        __syncthreads();
        unsigned long long s = 0ull, e = 0ull;
        for (int k = 0; k < waves; ++k) {
            s += slot[0][0][k];
            e += slot[0][1][k];
        }
        e >>= 1;   // every edge was counted from both ends
        unsigned long long h = wl_mix((unsigned long long)n * kWlSize + e);
        h = wl_mix(h + s);
        for (int t = 1; t <= iterations; ++t) {
            acc = 0ull;
            for (int i = wave; i < n; i += waves) {
                const unsigned long long* row = bitmap + (n0 + i) * W;
                const unsigned long long sum = wl_neighbour_sum(row, words, n, cur, lane);
                const unsigned long long c = wl_mix(cur[i] * kWlC + sum + (unsigned long long)t);
                if (lane == 0) nxt[i] = c;
                acc += wl_mix(c ^ kWlA);
            }
            if (lane == 0) slot[t & 1][0][wave] = acc;
            __syncthreads();   // the round's one barrier: nxt and the slots of this parity are complete
            s = 0ull;
            for (int k = 0; k < waves; ++k) s += slot[t & 1][0][k];
            h = wl_mix(h * kWlD + s);
            unsigned long long* swap = cur;
            cur = nxt;
            nxt = swap;
        }
        for (int i = tid; i < n; i += blockDim.x) node_colour[n0 + i] = cur[i];
        if (tid == 0) {
            hash[g] = h;
            n_edges[g] = (int64_t)e;
        }
    }
}

// ---- global route ----------------------------------------------------------------------------------------------------------
// a wave per row: colour 0 into `out`, its term into table[0][g], its degree into n_edges[g] (a degree sum until k_wl_fold)
__global__ __launch_bounds__(256) void k_wl_init(const int32_t* __restrict__ off, int64_t n_nodes, int cap, int64_t W,
                                                 const unsigned long long* __restrict__ bitmap,
                                                 const int32_t* __restrict__ gid, const int64_t* __restrict__ labels,
                                                 unsigned long long* __restrict__ out, unsigned long long* __restrict__ table,
                                                 unsigned long long* __restrict__ degree_sum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_nodes; i += (int64_t)gridDim.x * 4) {
        int g, n;
        int64_t n0;
        if (!graph_of_row(off, gid, n_nodes, cap, i, g, n0, n)) continue;   // (uniform over the wave)
        const unsigned long long* row = bitmap + i * W;
        unsigned long long d = 0ull;
        for (int w = lane; w < (n + 63) / 64; w += 64) d += __popcll(wl_row_word(row, w, n));
        d = wave_sum_u64(d);
        const unsigned long long c = wl_mix(labels ? (unsigned long long)labels[i] : d);
        if (lane == 0) {
            out[i] = c;
            atomicAdd(&table[g], wl_mix(c ^ kWlA));
            atomicAdd(&degree_sum[g], d);
        }
    }
}

// round t, a wave per row: out[i] from in[], its term into table[t][g]
__global__ __launch_bounds__(256) void k_wl_round(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes, int cap,
                                                  int64_t W, const unsigned long long* __restrict__ bitmap,
                                                  const int32_t* __restrict__ gid, int t,
                                                  const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                  unsigned long long* __restrict__ table) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_nodes; i += (int64_t)gridDim.x * 4) {
        int g, n;
        int64_t n0;
        if (!graph_of_row(off, gid, n_nodes, cap, i, g, n0, n)) continue;   // (uniform over the wave)
        const unsigned long long* row = bitmap + i * W;
        const unsigned long long sum = wl_neighbour_sum(row, (n + 63) / 64, n, in + n0, lane);
        const unsigned long long c = wl_mix(in[i] * kWlC + sum + (unsigned long long)t);
        if (lane == 0) {
            out[i] = c;
            atomicAdd(&table[(int64_t)t * n_graphs + g], wl_mix(c ^ kWlA));
        }
    }
}

// a thread per graph: e = degree sum / 2, h folded from the table in round order
__global__ __launch_bounds__(256) void k_wl_fold(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes, int cap,
                                                 int iterations, const unsigned long long* __restrict__ table,
                                                 unsigned long long* __restrict__ hash, int64_t* __restrict__ n_edges) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_graphs; g += (int64_t)gridDim.x * 256) {
        int64_t n0;
        int n;
        stats_graph_range(off, (int)g, n_nodes, cap, n0, n);
        const unsigned long long e = (unsigned long long)n_edges[g] >> 1;
        unsigned long long h = wl_mix((unsigned long long)n * kWlSize + e);
        h = wl_mix(h + table[g]);
        for (int t = 1; t <= iterations; ++t) h = wl_mix(h * kWlD + table[(int64_t)t * n_graphs + g]);
        hash[g] = h;
        n_edges[g] = (int64_t)e;
    }
}

// ---- matching --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_min_i32(int v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(v, o, 64);
        v = other < v ? other : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_hash_match(const unsigned long long* __restrict__ hash_a,
                                                    const int32_t* __restrict__ n_node_a, int64_t a,
                                                    const unsigned long long* __restrict__ hash_b,
                                                    const int32_t* __restrict__ n_node_b, int64_t b,
                                                    int32_t* __restrict__ first_in_a, int32_t* __restrict__ match_in_b,
                                                    unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < a; g += (int64_t)gridDim.x * 4) {
        const int32_t n = n_node_a[g];
        if (n == 0) {   // (uniform over the wave) left out
            if (lane == 0) {
                first_in_a[g] = -1;
                match_in_b[g] = -1;
            }
            continue;
        }
        const unsigned long long key = hash_a[g];
        int first = (int)g, match = 0x7fffffff;
        for (int64_t j = lane; j < g; j += 64)
            if (hash_a[j] == key && n_node_a[j] == n && j < first) first = (int)j;
        for (int64_t j = lane; j < b; j += 64)
            if (hash_b[j] == key && n_node_b[j] == n && j < match) match = (int)j;
        first = wave_min_i32(first);
        match = wave_min_i32(match);
        if (lane == 0) {
            const bool distinct = first == (int)g, novel = match == 0x7fffffff;
            first_in_a[g] = first;
            match_in_b[g] = novel ? -1 : match;
            atomicAdd(&counts[0], 1ull);
            if (distinct) atomicAdd(&counts[1], 1ull);
            if (novel) atomicAdd(&counts[2], 1ull);
            if (distinct && novel) atomicAdd(&counts[3], 1ull);
        }
    }
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_graph_hashes_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_graphs > 0x7fffffff || n_nodes < 0 || n_nodes > 0x7fffffff || max_nodes_per_graph < 0 ||
        max_nodes_per_graph > kWlMaxNodes)
        return 0;
    return wl_ws(n_graphs, n_nodes, max_nodes_per_graph).total;
}

int gnf_graph_hashes(const GnfCsr* csr, int32_t max_nodes_per_graph, int32_t iterations, const int64_t* labels, uint64_t* hash,
                     uint64_t* node_colour, int64_t* n_edges, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_graph_hashes";
    if (int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kWlMaxNodes, "gnf_graph_stats' limit")) return rc;
    if (csr->n_nodes > 0x7fffffff) {
        set_error("%s: n_nodes=%lld does not fit the int32 node ids", what, (long long)csr->n_nodes);
        return GNF_ESHAPE;
    }
    if (iterations < 0 || iterations > kWlMaxIter) {
        set_error("%s: iterations=%d (0 <= iterations <= %d)", what, iterations, kWlMaxIter);
        return GNF_ESHAPE;
    }
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    if ((n > 0 && (!node_colour || !ws)) || (b > 0 && (!hash || !n_edges))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const int cap = max_nodes_per_graph;
    const WlWs L = wl_ws(b, n, cap);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    if (b == 0) return GNF_OK;   // an empty batch: nothing to write
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* hash64 = (unsigned long long*)hash;
    unsigned long long* colour = (unsigned long long*)node_colour;
    if (n == 0) {                // graphs without nodes: the hash of n = e = 0, no bitmap, no LDS
        hipLaunchKernelGGL(k_wl_lds, dim3(stats_grid(b)), dim3(256), 0, st, csr->node_offsets, b, n, 0, (int64_t)0,
                           (const unsigned long long*)nullptr, labels, iterations, hash64, colour, n_edges);
        GNF_LAUNCH_CHECK("k_wl_lds");
        return GNF_OK;
    }
    char* base = (char*)ws;
    unsigned long long* bitmap = (unsigned long long*)(base + L.stats.bitmap);
    int32_t* gid = (int32_t*)(base + L.stats.gid);
    GNF_HIP_TRY(hipMemsetAsync(node_colour, 0, (size_t)n * sizeof(uint64_t), st));   // rows no graph (or no column) covers: 0
    if (int rc = build_graph_bitmap(csr, cap, L.stats.W, bitmap, gid, st)) return rc;
    if (cap <= kWlLdsNodes) {
        const size_t lds = 2 * (size_t)cap * sizeof(uint64_t);   // <= 64 KiB, + 512 bytes of static slots
        GNF_ONCE_PER_DEVICE(GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_wl_lds),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize,
                                                            2 * kWlLdsNodes * (int)sizeof(uint64_t))));
        hipLaunchKernelGGL(k_wl_lds, dim3(stats_grid(b)), dim3(cap <= 256 ? 256 : 64 * kWlMaxWaves), lds, st, csr->node_offsets,
                           b, n, cap, L.stats.W, bitmap, labels, iterations, hash64, colour, n_edges);
        GNF_LAUNCH_CHECK("k_wl_lds");
        return GNF_OK;
    }
    unsigned long long* buf[2] = {(unsigned long long*)(base + L.col_a), (unsigned long long*)(base + L.col_b)};
    unsigned long long* table = (unsigned long long*)(base + L.table);
    GNF_HIP_TRY(hipMemsetAsync(table, 0, (size_t)(iterations + 1) * (size_t)b * sizeof(uint64_t), st));
    GNF_HIP_TRY(hipMemsetAsync(n_edges, 0, (size_t)b * sizeof(int64_t), st));
    const dim3 rows(stats_grid((n + 3) / 4));
    // round t reads what round t - 1 wrote and writes buffer t & 1; the last round writes node_colour itself
    unsigned long long* out = iterations == 0 ? colour : buf[0];
    hipLaunchKernelGGL(k_wl_init, rows, dim3(256), 0, st, csr->node_offsets, n, cap, L.stats.W, bitmap, gid, labels, out, table,
                       (unsigned long long*)n_edges);
    GNF_LAUNCH_CHECK("k_wl_init");
    for (int t = 1; t <= iterations; ++t) {
        const unsigned long long* in = out;
        out = t == iterations ? colour : buf[t & 1];
        hipLaunchKernelGGL(k_wl_round, rows, dim3(256), 0, st, csr->node_offsets, b, n, cap, L.stats.W, bitmap, gid, t, in, out,
                           table);
        GNF_LAUNCH_CHECK("k_wl_round");
    }
    hipLaunchKernelGGL(k_wl_fold, dim3(stats_grid((b + 255) / 256)), dim3(256), 0, st, csr->node_offsets, b, n, cap, iterations,
                       table, hash64, n_edges);
    GNF_LAUNCH_CHECK("k_wl_fold");
    return GNF_OK;
}

size_t gnf_graph_hash_match_workspace_bytes(int64_t a, int64_t b) {
    if (a < 0 || b < 0 || a > 0x7fffffff || b > 0x7fffffff) return 0;
    return 8;   // one reserved word: the kernel needs none, and 0 says "no call accepts these arguments"
}

int gnf_graph_hash_match(const uint64_t* hash_a, const int32_t* n_node_a, int64_t a, const uint64_t* hash_b,
                         const int32_t* n_node_b, int64_t b, int32_t* first_in_a, int32_t* match_in_b, int64_t* counts, void* ws,
                         size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_graph_hash_match";
    if (a < 0 || b < 0 || a > 0x7fffffff || b > 0x7fffffff) {
        set_error("%s: a=%lld b=%lld (0 <= a, b <= INT32_MAX)", what, (long long)a, (long long)b);
        return GNF_ESHAPE;
    }
    if (!counts || !ws || (a > 0 && (!hash_a || !n_node_a || !first_in_a || !match_in_b)) || (b > 0 && (!hash_b || !n_node_b))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    if (ws_bytes < gnf_graph_hash_match_workspace_bytes(a, b)) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, gnf_graph_hash_match_workspace_bytes(a, b));
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    GNF_HIP_TRY(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st));
    if (a == 0) return GNF_OK;
    hipLaunchKernelGGL(k_hash_match, dim3(stats_grid((a + 3) / 4)), dim3(256), 0, st, (const unsigned long long*)hash_a, n_node_a,
                       a, (const unsigned long long*)hash_b, n_node_b, b, first_in_a, match_in_b, (unsigned long long*)counts);
    GNF_LAUNCH_CHECK("k_hash_match");
    return GNF_OK;
}

}  // extern "C"
