// Connected components of every graph of a batch and the extraction of a node-induced subgraph batch - the step between
// decode_graphs and the four scores (gnf_graph_stats / _orbits / _spectra): `pred_adj > threshold` decides every pair of nodes on
// its own, nothing makes the result one graph.  The reference stops at pickling the graphs (generate_graphs.py:68-84); nothing
// in it corresponds to these kernels.
//
// Graph model and bitmap: as in gnf_graph_stats.hip (undirected, simple), built by build_graph_bitmap (gnf_graph_bitmap.h:
// k_stats_bitmap on a zeroed bitmap).  A component is named by the batch-wide row of its smallest node: a definition, not a search order.
//
// gnf_graph_components.  k_stats_bitmap, then k_components - one workgroup of 256 threads per graph, striding over graphs;
// the bitmap rows stay in global memory, three bitsets of W = ceil(max_nodes / 64) words sit in LDS (visited | frontier | next,
// 24 W bytes <= 24 KiB):
//   1. a wave per row: an all-zero row is an isolated node - its own component of size 1, marked visited, counted.
//   2. searches, seeds in ascending node order (the smallest unvisited node, an LDS atomicMin over the words), so the seed IS the
//      component's root.  Per level: every wave walks the frontier's set bits, the k-th one belongs to wave k mod 4, whose lanes
//      take the row's words: next[w] |= row[w] & ~visited[w] (integer LDS atomics).  After a barrier thread t owns words t,
//      t + 256, ...: the new bits get the root as their label, the size counter grows by their popcount, visited |= next,
//      frontier = next, next = 0.  A level without a new bit ends the search; the root's size goes to the workspace.
//   3. component_size[i] = size of component[i]'s root; the per-graph figures from registers every thread carries alike.
// Loop bounds (binding): at most n_g searches per graph, at most n_g levels per search, whatever the bitmap holds - offsets or
// edge lists that do not describe the batch give wrong labels, never a hang or an access outside the arrays.
// Cost per graph: the bitmap is read twice, n_g W 8 bytes each (step 1; step 2 reads a row once, when its node is on the
// frontier), and every level pays one barrier pair - a path on n nodes numbered end to end costs n / 2 .. n levels.
// Integer atomics only (OR, MIN, ADD on integers): two calls give the same bits.
//
// gnf_graph_subgraph_count / _fill: the count -> scan -> fill scheme of gnf_decode_edges.hip on the rows of a keep set.
//   count: bitmap (and the components, for GNF_KEEP_LARGEST_COMPONENT; k_sub_degree_flags for GNF_KEEP_NON_ISOLATED);
//          k_sub_keep: per graph the keep bitset (a ballot per 64 columns) and the exclusive per-word ranks, new_n_node;
//          k_sub_offsets: new_off = exclusive scan of new_n_node, N';  k_sub_rows: a wave per old row - new_id, and the kept
//          row's degree sum_w popc(row[w] & keep[w]) (+ 1 with self_loops) stored at its NEW row;  k_sub_scan: rowptr, n_edge, E'.
//   fill:  k_sub_fill, a wave per old row, lane = column: new sender = new_off[g] + rank[w] + popc(keep[w] & below-lane), the
//          loop (self_loops) is the row's own bit ORed into its word, so it lands at its sorted place.  Vector stores only; every
//          word, count, id and edge has exactly one writer.
// A graph's keep / rank words start at word (n0 >> 6) + g of arrays of n_nodes / 64 + n_graphs + 1 words: disjoint for
// ascending offsets (floor(a / 64) + floor(b / 64) <= floor((a + b) / 64)), inside the arrays for any offsets.
#include "gnf_graph_bitmap.h"

namespace gnf {

static constexpr int kCompMaxNodes = GNF_COMPONENTS_MAX_NODES;
static constexpr int kCompBlock = 256, kCompWaves = kCompBlock / 64;

static inline size_t up8(size_t v) { return (v + 7) / 8 * 8; }

// caller-owned workspace of gnf_graph_components (host only): the gnf_graph_stats workspace (bitmap, gid) | root_size int32 [N]
struct CompWs {
    StatsWs stats;
    size_t root_size, total;
};
static CompWs comp_ws(int64_t n_nodes, int32_t cap) {
    CompWs L;
    L.stats = stats_ws(n_nodes, cap);
    L.root_size = L.stats.total;
    L.total = up8(L.root_size + (size_t)n_nodes * sizeof(int32_t));
    return L;
}

// caller-owned workspace of gnf_graph_subgraph_count / _fill (host only): the gnf_graph_components workspace | keep uint64 [KW] |
// rank int32 [KW] | component, component_size, new_id, rowcnt int32 [N] each | n_components, largest_size, largest_root,
// n_isolated int32 [B] each | off, new_off int32 [B + 1] each | flags uint8 [N] | hdr int32 [2] {self_loops, -};  KW = N / 64 + B + 1
struct SubWs {
    CompWs comp;
    size_t keep, rank, component, component_size, new_id, rowcnt, per_graph, off, new_off, flags, hdr, total;
    int64_t KW;
};
static SubWs sub_ws(int64_t n_graphs, int64_t n_nodes, int32_t cap) {
    SubWs L;
    L.comp = comp_ws(n_nodes, cap);
    L.KW = n_nodes / 64 + n_graphs + 1;
    const size_t nodes4 = up8((size_t)n_nodes * sizeof(int32_t)), graphs4 = up8((size_t)(n_graphs + 1) * sizeof(int32_t));
    L.keep = L.comp.total;
    L.rank = L.keep + (size_t)L.KW * sizeof(uint64_t);
    L.component = L.rank + up8((size_t)L.KW * sizeof(int32_t));
    L.component_size = L.component + nodes4;
    L.new_id = L.component_size + nodes4;
    L.rowcnt = L.new_id + nodes4;
    L.per_graph = L.rowcnt + nodes4;
    L.off = L.per_graph + 4 * graphs4;
    L.new_off = L.off + graphs4;
    L.flags = L.new_off + graphs4;
    L.hdr = L.flags + up8((size_t)n_nodes);
    L.total = L.hdr + 8;
    return L;
}

// ---- components ------------------------------------------------------------------------------------------------------------
// LDS: visited [W] | frontier [W] | next [W] 64-bit words | ctl int32 [8]: seed, size, n_isolated, (unused), more[2]
__global__ __launch_bounds__(kCompBlock) void k_components(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes,
                                                           int cap, int64_t W, const unsigned long long* __restrict__ bitmap,
                                                           int32_t* component, int32_t* __restrict__ component_size,
                                                           int32_t* __restrict__ n_components, int32_t* __restrict__ largest_size,
                                                           int32_t* __restrict__ largest_root, int32_t* __restrict__ n_isolated,
                                                           int32_t* root_size) {
    extern __shared__ unsigned long long comp_lds[];
    unsigned long long* visited = comp_lds;
    unsigned long long* frontier = visited + W;
    unsigned long long* next = frontier + W;
    int32_t* ctl = (int32_t*)(next + W);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int64_t g = blockIdx.x; g < n_graphs; g += gridDim.x) {   // (uniform over the workgroup)
        int64_t n0;
        int n;
        stats_graph_range(off, (int)g, n_nodes, cap, n0, n);
        const int words = (n + 63) / 64;
        __syncthreads();   // the previous graph's readers are done
        for (int w = tid; w < words; w += kCompBlock) {
            const int tail = n - w * 64;   // columns of this word inside the graph; the others count as visited
            visited[w] = tail >= 64 ? 0ull : ~((1ull << tail) - 1ull);
            frontier[w] = 0ull;
            next[w] = 0ull;
        }
        if (tid < 8) ctl[tid] = 0;
        __syncthreads();
        // 1. isolated nodes
        for (int i = wave; i < n; i += kCompWaves) {
            const unsigned long long* row = bitmap + (n0 + i) * W;
            unsigned long long any = 0ull;
            for (int w = lane; w < words; w += 64) any |= row[w];
            if (__ballot(any != 0ull) == 0ull && lane == 0) {
                atomicOr(&visited[i >> 6], 1ull << (i & 63));
                atomicAdd(&ctl[2], 1);
                component[n0 + i] = (int32_t)(n0 + i);
                root_size[n0 + i] = 1;
            }
        }
        __syncthreads();
        const int isolated = ctl[2];
        int searches = 0, best = 0, best_root = -1;   // (the same in every thread)
        // 2. searches: at most n of them, at most n levels each
        for (int s = 0; s < n; ++s) {
            if (tid == 0) ctl[0] = 0x7fffffff;
            __syncthreads();
            for (int w = tid; w < words; w += kCompBlock) {
                const unsigned long long open = ~visited[w];
                if (open) atomicMin(&ctl[0], w * 64 + __ffsll((long long)open) - 1);
            }
            __syncthreads();
            const int seed = ctl[0];
            if (seed >= n) break;   // (uniform) every node has its label
            const int32_t root = (int32_t)(n0 + seed);
            if (tid == 0) {
                visited[seed >> 6] |= 1ull << (seed & 63);
                frontier[seed >> 6] = 1ull << (seed & 63);
                ctl[1] = 1;
                ctl[4] = 0;
                ctl[5] = 0;
                component[root] = root;
            }
            __syncthreads();
            for (int lvl = 0; lvl < n; ++lvl) {
                // expand: the k-th frontier node goes to wave k mod kCompWaves
                int k = 0;
                for (int f0 = 0; f0 < words; f0 += 64) {
                    const unsigned long long mine = f0 + lane < words ? frontier[f0 + lane] : 0ull;
                    unsigned long long busy = __ballot(mine != 0ull);
                    while (busy) {
                        const int l = __ffsll((long long)busy) - 1;
                        busy &= busy - 1ull;
                        unsigned long long word = __shfl(mine, l, 64);
                        while (word) {
                            const int i = (f0 + l) * 64 + __ffsll((long long)word) - 1;
                            word &= word - 1ull;
                            if ((k++ & (kCompWaves - 1)) != wave) continue;
                            const unsigned long long* row = bitmap + (n0 + i) * W;
                            for (int w = lane; w < words; w += 64) {
                                const unsigned long long fresh = row[w] & ~visited[w];
                                if (fresh) atomicOr(&next[w], fresh);
                            }
                        }
                    }
                }
                __syncthreads();
                // label: thread t owns words t, t + 256, ...
                if (tid == 0) ctl[4 + ((lvl + 1) & 1)] = 0;
                int grown = 0;
                for (int w = tid; w < words; w += kCompBlock) {
                    const unsigned long long fresh = next[w] & ~visited[w];
                    frontier[w] = fresh;
                    next[w] = 0ull;
                    if (!fresh) continue;
                    visited[w] |= fresh;
                    grown += __popcll(fresh);
                    for (unsigned long long bits = fresh; bits; bits &= bits - 1ull)
                        component[n0 + w * 64 + __ffsll((long long)bits) - 1] = root;
                }
                if (grown) {
                    atomicAdd(&ctl[1], grown);
                    atomicOr(&ctl[4 + (lvl & 1)], 1);
                }
                __syncthreads();
                if (!ctl[4 + (lvl & 1)]) break;   // (uniform)
            }
            const int size = ctl[1];   // (its next writer waits behind the two barriers that open the next search)
            if (tid == 0) root_size[root] = size;
            ++searches;
            if (size > best) {   // seeds ascend: a tie keeps the smaller root
                best = size;
                best_root = root;
            }
        }
        if (best == 0 && isolated > 0) {   // nothing but isolated nodes: the first of them
            best = 1;
            best_root = (int32_t)n0;
        }
        __syncthreads();   // the labels and root sizes of this workgroup are visible to it
        // 3. sizes
        for (int i = tid; i < n; i += kCompBlock) {
            const int64_t c = component[n0 + i];
            component_size[n0 + i] = c >= 0 && c < n_nodes ? root_size[c] : 0;
        }
        if (tid == 0) {
            n_components[g] = searches + isolated;
            largest_size[g] = best;
            largest_root[g] = best_root;
            n_isolated[g] = isolated;
        }
    }
}

// ---- extraction ------------------------------------------------------------------------------------------------------------
// flags[i] = 1 for a row with a neighbour (a wave per row), 0 otherwise - GNF_KEEP_NON_ISOLATED as a mask
__global__ __launch_bounds__(256) void k_sub_degree_flags(const int32_t* __restrict__ off, int64_t n_nodes, int cap, int64_t W,
                                                          const unsigned long long* __restrict__ bitmap,
                                                          const int32_t* __restrict__ gid, uint8_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_nodes; i += (int64_t)gridDim.x * 4) {
        int g, n;
        int64_t n0;
        unsigned long long any = 0ull;
        if (graph_of_row(off, gid, n_nodes, cap, i, g, n0, n))
            for (int w = lane; w < (n + 63) / 64; w += 64) any |= bitmap[i * W + w];
        const bool has = __ballot(any != 0ull) != 0ull;
        if (lane == 0) flags[i] = has ? 1 : 0;
    }
}

// one workgroup per graph: keep words by ballot (wave per 64 columns), then their exclusive ranks in place
__global__ __launch_bounds__(256) void k_sub_keep(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes, int cap,
                                                  int rule, const uint8_t* __restrict__ mask,
                                                  const int32_t* __restrict__ component,
                                                  const int32_t* __restrict__ largest_root,
                                                  unsigned long long* __restrict__ keep, int32_t* rank,
                                                  int32_t* __restrict__ new_n_node) {
    __shared__ int32_t sh[257];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t g = blockIdx.x; g < n_graphs; g += gridDim.x) {   // (uniform over the workgroup)
        int64_t n0;
        int n;
        stats_graph_range(off, (int)g, n_nodes, cap, n0, n);
        const int words = (n + 63) / 64;
        const int64_t kw = (n0 >> 6) + g;
        const int32_t root = rule == GNF_KEEP_LARGEST_COMPONENT ? largest_root[g] : -1;
        __syncthreads();   // the previous graph's readers of sh are done
        for (int w = wave; w < words; w += 4) {
            const int j = w * 64 + lane;
            bool k = false;
            if (j < n) k = rule == GNF_KEEP_LARGEST_COMPONENT ? (root >= 0 && component[n0 + j] == root) : mask[n0 + j] != 0;
            const unsigned long long word = __ballot(k);
            if (lane == 0) {
                keep[kw + w] = word;
                rank[kw + w] = __popcll(word);
            }
        }
        __syncthreads();
        const int chunk = (words + 255) / 256;
        const int beg = tid * chunk, end = beg + chunk < words ? beg + chunk : words;
        int32_t l = 0;
        for (int w = beg; w < end; ++w) l += rank[kw + w];
        sh[tid + 1] = l;
        if (tid == 0) sh[0] = 0;
        __syncthreads();
        if (tid == 0)
            for (int i = 1; i <= 256; ++i) sh[i] += sh[i - 1];
        __syncthreads();
        int32_t r = sh[tid];
        for (int w = beg; w < end; ++w) {
            const int32_t c = rank[kw + w];
            rank[kw + w] = r;
            r += c;
        }
        if (tid == 0) new_n_node[g] = sh[256];
    }
}

// new_off = exclusive scan of new_n_node (one workgroup, a contiguous chunk of graphs per thread: any B); the offsets and
// self_loops are kept for the fill, totals[0] = N'
__global__ __launch_bounds__(256) void k_sub_offsets(const int32_t* __restrict__ off, const int32_t* __restrict__ new_n_node,
                                                     int64_t n_graphs, int self_loops, int32_t* __restrict__ off_copy,
                                                     int32_t* __restrict__ new_off, int32_t* __restrict__ hdr,
                                                     int64_t* __restrict__ totals) {
    __shared__ int64_t sh[257];
    const int64_t chunk = (n_graphs + 255) / 256;
    const int64_t beg = (int64_t)threadIdx.x * chunk;
    int64_t end = beg + chunk;
    if (end > n_graphs) end = n_graphs;
    int64_t l = 0;
    for (int64_t i = beg; i < end; ++i) l += new_n_node[i];
    sh[threadIdx.x + 1] = l;
    if (threadIdx.x == 0) sh[0] = 0;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i <= 256; ++i) sh[i] += sh[i - 1];
    __syncthreads();
    int64_t r = sh[threadIdx.x];
    if (threadIdx.x == 0) {
        new_off[0] = 0;
        off_copy[0] = off[0];
        hdr[0] = self_loops;
        hdr[1] = 0;
        totals[0] = sh[256];
    }
    for (int64_t i = beg; i < end; ++i) {
        r += new_n_node[i];
        new_off[i + 1] = (int32_t)r;
        off_copy[i + 1] = off[i + 1];
    }
}

// the new row of old row i (graph g, local li), -1 for a row that is not kept or that no graph covers
__device__ __forceinline__ int32_t sub_new_row(const unsigned long long* __restrict__ keep, const int32_t* __restrict__ rank,
                                               const int32_t* __restrict__ new_off, int g, int64_t n0, int64_t li) {
    const int64_t kw = (n0 >> 6) + g + (li >> 6);
    const unsigned long long word = keep[kw];
    if (!((word >> (li & 63)) & 1ull)) return -1;
    return new_off[g] + rank[kw] + __popcll(word & ((1ull << (li & 63)) - 1ull));
}

// a wave per old row: new_id, and the degree of a kept row at its new row
__global__ __launch_bounds__(256) void k_sub_rows(const int32_t* __restrict__ off, int64_t n_nodes, int cap, int64_t W,
                                                  int self_loops, const unsigned long long* __restrict__ bitmap,
                                                  const int32_t* __restrict__ gid, const unsigned long long* __restrict__ keep,
                                                  const int32_t* __restrict__ rank, const int32_t* __restrict__ new_off,
                                                  int32_t* __restrict__ new_id, int32_t* __restrict__ new_id_ws,
                                                  int32_t* __restrict__ rowcnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_nodes; i += (int64_t)gridDim.x * 4) {
        int g, n;
        int64_t n0;
        int32_t r = -1;
        if (graph_of_row(off, gid, n_nodes, cap, i, g, n0, n)) r = sub_new_row(keep, rank, new_off, g, n0, i - n0);
        if (r >= n_nodes) r = -1;   // (offsets that do not describe the batch)
        if (lane == 0) {
            new_id[i] = r;
            new_id_ws[i] = r;
        }
        if (r < 0) continue;
        const int64_t kw = (n0 >> 6) + g;
        unsigned long long d = 0;
        for (int w = lane; w < (n + 63) / 64; w += 64) d += __popcll(bitmap[i * W + w] & keep[kw + w]);
        d = wave_sum_u64(d);
        if (lane == 0) rowcnt[r] = (int32_t)d + (self_loops ? 1 : 0);
    }
}

// rowptr = exclusive prefix of rowcnt over the N' = new_off[n_graphs] new rows, then n_edge and totals[1] = E' (one workgroup;
// n_nodes * (max_nodes + 1) <= INT32_MAX, checked on the host, bounds every sum)
__global__ __launch_bounds__(256) void k_sub_scan(const int32_t* __restrict__ rowcnt, int64_t n_nodes,
                                                  const int32_t* __restrict__ new_off, int64_t n_graphs, int32_t* rowptr,
                                                  int32_t* __restrict__ n_edge, int64_t* __restrict__ totals) {
    __shared__ int32_t sh[257];
    int64_t rows = new_off[n_graphs];
    rows = rows < 0 ? 0 : (rows > n_nodes ? n_nodes : rows);
    const int64_t chunk = (rows + 255) / 256;
    const int64_t beg = (int64_t)threadIdx.x * chunk;
    int64_t end = beg + chunk;
    if (end > rows) end = rows;
    int32_t l = 0;
    for (int64_t i = beg; i < end; ++i) l += rowcnt[i];
    sh[threadIdx.x + 1] = l;
    if (threadIdx.x == 0) sh[0] = 0;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i <= 256; ++i) sh[i] += sh[i - 1];
    __syncthreads();
    int32_t r = sh[threadIdx.x];
    if (threadIdx.x == 0) {
        rowptr[0] = 0;
        totals[1] = sh[256];
    }
    for (int64_t i = beg; i < end; ++i) {
        r += rowcnt[i];
        rowptr[i + 1] = r;
    }
    __syncthreads();   // rowptr written above is read below by other threads of this workgroup
    for (int64_t g = threadIdx.x; g < n_graphs; g += 256) {
        int64_t a = new_off[g], b = new_off[g + 1];
        a = a < 0 ? 0 : (a > rows ? rows : a);
        b = b < a ? a : (b > rows ? rows : b);
        n_edge[g] = rowptr[b] - rowptr[a];
    }
}

// pass 2: a wave per old row; lane = column of the current word.  Ids >= a capacity are dropped.
__global__ __launch_bounds__(256) void k_sub_fill(const int32_t* __restrict__ off, int64_t n_graphs, int64_t n_nodes, int cap,
                                                  int64_t W, const unsigned long long* __restrict__ bitmap,
                                                  const int32_t* __restrict__ gid, const unsigned long long* __restrict__ keep,
                                                  const int32_t* __restrict__ rank, const int32_t* __restrict__ new_off,
                                                  const int32_t* __restrict__ new_id, const int32_t* __restrict__ hdr,
                                                  const int32_t* __restrict__ rowptr, int64_t node_capacity,
                                                  int64_t edge_capacity, int32_t* __restrict__ node_index,
                                                  int32_t* __restrict__ senders, int32_t* __restrict__ receivers) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int self_loops = hdr[0];
    for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n_nodes; i += (int64_t)gridDim.x * 4) {
        const int64_t r = new_id[i];
        const int g = gid[i];
        if (r < 0 || r >= n_nodes || g < 0 || g >= n_graphs) continue;
        int64_t n0;
        int n;
        stats_graph_range(off, g, n_nodes, cap, n0, n);
        const int64_t li = i - n0;
        if (li < 0 || li >= n) continue;
        if (lane == 0 && r < node_capacity) node_index[r] = (int32_t)i;
        const int64_t kw = (n0 >> 6) + g;
        const int64_t base = new_off[g];
        int64_t e0 = rowptr[r];
        for (int w = 0; w < (n + 63) / 64 && e0 >= 0 && e0 < edge_capacity; ++w) {
            const unsigned long long kept = keep[kw + w];
            unsigned long long word = bitmap[i * W + w] & kept;
            if (self_loops && w == (int)(li >> 6)) word |= 1ull << (li & 63);
            const unsigned long long below = (1ull << lane) - 1ull;
            const int64_t e = e0 + __popcll(word & below);
            if (((word >> lane) & 1ull) && e < edge_capacity) {
                senders[e] = (int32_t)(base + rank[kw + w] + __popcll(kept & below));
                receivers[e] = (int32_t)r;
            }
            e0 += __popcll(word);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static bool sub_sizes_ok(int64_t n_graphs, int64_t n_nodes, int32_t cap) {
    return n_graphs >= 0 && n_graphs <= 0x7fffffff && n_nodes >= 0 && cap >= 0 && cap <= kCompMaxNodes &&
           n_nodes * ((int64_t)cap + 1) <= INT32_MAX;
}

// bitmap + components of a validated batch with nodes (n > 0, b > 0)
static int launch_components(const GnfCsr* csr, int32_t cap, const CompWs& L, void* ws, int32_t* component,
                             int32_t* component_size, int32_t* n_components, int32_t* largest_size, int32_t* largest_root,
                             int32_t* n_isolated, bool search, hipStream_t st) {
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    unsigned long long* bitmap = (unsigned long long*)((char*)ws + L.stats.bitmap);
    int32_t* gid = (int32_t*)((char*)ws + L.stats.gid);
    if (int rc = build_graph_bitmap(csr, cap, L.stats.W, bitmap, gid, st)) return rc;
    if (!search) return GNF_OK;
    GNF_HIP_TRY(hipMemsetAsync(component, 0xff, (size_t)n * sizeof(int32_t), st));   // rows no graph (or no column) covers: -1
    GNF_HIP_TRY(hipMemsetAsync(component_size, 0, (size_t)n * sizeof(int32_t), st));
    const size_t lds = 3 * (size_t)L.stats.W * sizeof(uint64_t) + 8 * sizeof(int32_t);   // <= 24 KiB + 32
    hipLaunchKernelGGL(k_components, dim3(stats_grid(b)), dim3(kCompBlock), lds, st, csr->node_offsets, b, n, cap, L.stats.W,
                       bitmap, component, component_size, n_components, largest_size, largest_root, n_isolated,
                       (int32_t*)((char*)ws + L.root_size));
    GNF_LAUNCH_CHECK("k_components");
    return GNF_OK;
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_graph_components_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (n_graphs < 0 || n_nodes < 0 || n_nodes > 0x7fffffff || max_nodes_per_graph < 0 || max_nodes_per_graph > kCompMaxNodes)
        return 0;
    return comp_ws(n_nodes, max_nodes_per_graph).total;
}

int gnf_graph_components(const GnfCsr* csr, int32_t max_nodes_per_graph, int32_t* component, int32_t* component_size,
                         int32_t* n_components, int32_t* largest_size, int32_t* largest_root, int32_t* n_isolated, void* ws,
                         size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_graph_components";
    if (int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kCompMaxNodes, "gnf_graph_stats' limit")) return rc;
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    if (n > 0x7fffffff) {
        set_error("%s: n_nodes=%lld does not fit the int32 node ids", what, (long long)n);
        return GNF_ESHAPE;
    }
    if ((n > 0 && (!component || !component_size || !ws)) ||
        (b > 0 && (!n_components || !largest_size || !largest_root || !n_isolated))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    const CompWs L = comp_ws(n, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    if (b == 0) return GNF_OK;   // an empty batch: nothing to write
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {                // graphs without nodes
        GNF_HIP_TRY(hipMemsetAsync(n_components, 0, (size_t)b * sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(largest_size, 0, (size_t)b * sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(largest_root, 0xff, (size_t)b * sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(n_isolated, 0, (size_t)b * sizeof(int32_t), st));
        return GNF_OK;
    }
    return launch_components(csr, max_nodes_per_graph, L, ws, component, component_size, n_components, largest_size, largest_root,
                             n_isolated, true, st);
}

size_t gnf_graph_subgraph_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph) {
    if (!sub_sizes_ok(n_graphs, n_nodes, max_nodes_per_graph)) return 0;
    return sub_ws(n_graphs, n_nodes, max_nodes_per_graph).total;
}

int gnf_graph_subgraph_count(const GnfCsr* csr, int32_t max_nodes_per_graph, int32_t rule, const uint8_t* mask,
                             int32_t self_loops, int32_t* new_id, int32_t* new_n_node, int32_t* rowptr, int32_t* n_edge,
                             int64_t* totals, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_graph_subgraph_count";
    if (int rc = graph_csr_ok(what, csr, max_nodes_per_graph, kCompMaxNodes, "gnf_graph_stats' limit")) return rc;
    const int64_t n = csr->n_nodes, b = csr->n_graphs;
    if (!sub_sizes_ok(b, n, max_nodes_per_graph)) {
        set_error("%s: n_nodes=%lld x (max_nodes_per_graph=%d + 1) exceeds the int32 edge ids", what, (long long)n,
                  max_nodes_per_graph);
        return GNF_ESHAPE;
    }
    if (rule != GNF_KEEP_LARGEST_COMPONENT && rule != GNF_KEEP_NON_ISOLATED && rule != GNF_KEEP_MASK) {
        set_error("%s: rule=%d", what, rule);
        return GNF_EINVAL;
    }
    if (self_loops != 0 && self_loops != 1) {
        set_error("%s: self_loops=%d (0 or 1)", what, self_loops);
        return GNF_EINVAL;
    }
    if (rule == GNF_KEEP_MASK && !mask) {
        set_error("%s: GNF_KEEP_MASK with a null mask", what);
        return GNF_EINVAL;
    }
    if ((n > 0 && (!new_id || !ws)) || (b > 0 && (!new_n_node || !rowptr || !n_edge || !totals))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    if (b == 0) return GNF_OK;   // an empty batch: nothing to write, no workspace to read
    const SubWs L = sub_ws(b, n, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {                // graphs without nodes: nothing kept
        GNF_HIP_TRY(hipMemsetAsync(new_n_node, 0, (size_t)b * sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(n_edge, 0, (size_t)b * sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(rowptr, 0, sizeof(int32_t), st));
        GNF_HIP_TRY(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
        return GNF_OK;
    }
    char* base = (char*)ws;
    const int cap = max_nodes_per_graph;
    const size_t graphs4 = up8((size_t)(b + 1) * sizeof(int32_t));
    const unsigned long long* bitmap = (const unsigned long long*)(base + L.comp.stats.bitmap);
    const int32_t* gid = (const int32_t*)(base + L.comp.stats.gid);
    int32_t* component = (int32_t*)(base + L.component);
    int32_t* per_graph = (int32_t*)(base + L.per_graph);
    int32_t* largest_root = (int32_t*)(base + L.per_graph + 2 * graphs4);
    uint8_t* flags = (uint8_t*)(base + L.flags);
    unsigned long long* keep = (unsigned long long*)(base + L.keep);
    int32_t* rank = (int32_t*)(base + L.rank);
    int32_t* new_off = (int32_t*)(base + L.new_off);
    if (int rc = launch_components(csr, cap, L.comp, ws, component, (int32_t*)(base + L.component_size), per_graph,
                                   (int32_t*)(base + L.per_graph + graphs4), largest_root,
                                   (int32_t*)(base + L.per_graph + 3 * graphs4), rule == GNF_KEEP_LARGEST_COMPONENT, st))
        return rc;
    if (rule == GNF_KEEP_NON_ISOLATED) {
        hipLaunchKernelGGL(k_sub_degree_flags, dim3(stats_grid((n + 3) / 4)), dim3(256), 0, st, csr->node_offsets, n, cap,
                           L.comp.stats.W, bitmap, gid, flags);
        GNF_LAUNCH_CHECK("k_sub_degree_flags");
        mask = flags;
    }
    hipLaunchKernelGGL(k_sub_keep, dim3(stats_grid(b)), dim3(256), 0, st, csr->node_offsets, b, n, cap, rule, mask, component,
                       largest_root, keep, rank, new_n_node);
    GNF_LAUNCH_CHECK("k_sub_keep");
    hipLaunchKernelGGL(k_sub_offsets, dim3(1), dim3(256), 0, st, csr->node_offsets, new_n_node, b, self_loops,
                       (int32_t*)(base + L.off), new_off, (int32_t*)(base + L.hdr), totals);
    GNF_LAUNCH_CHECK("k_sub_offsets");
    hipLaunchKernelGGL(k_sub_rows, dim3(stats_grid((n + 3) / 4)), dim3(256), 0, st, csr->node_offsets, n, cap, L.comp.stats.W,
                       self_loops, bitmap, gid, keep, rank, new_off, new_id, (int32_t*)(base + L.new_id),
                       (int32_t*)(base + L.rowcnt));
    GNF_LAUNCH_CHECK("k_sub_rows");
    hipLaunchKernelGGL(k_sub_scan, dim3(1), dim3(256), 0, st, (const int32_t*)(base + L.rowcnt), n, new_off, b, rowptr, n_edge,
                       totals);
    GNF_LAUNCH_CHECK("k_sub_scan");
    return GNF_OK;
}

int gnf_graph_subgraph_fill(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph, const int32_t* rowptr,
                            int64_t node_capacity, int64_t edge_capacity, int32_t* node_index, int32_t* senders,
                            int32_t* receivers, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_graph_subgraph_fill";
    if (!sub_sizes_ok(n_graphs, n_nodes, max_nodes_per_graph) || node_capacity < 0 || edge_capacity < 0 ||
        (n_nodes > 0 && n_graphs > 0 && max_nodes_per_graph == 0)) {
        set_error("%s: n_graphs=%lld n_nodes=%lld max_nodes_per_graph=%d node_capacity=%lld edge_capacity=%lld", what,
                  (long long)n_graphs, (long long)n_nodes, max_nodes_per_graph, (long long)node_capacity,
                  (long long)edge_capacity);
        return GNF_ESHAPE;
    }
    const bool work = n_graphs > 0 && n_nodes > 0;
    if (work && (!rowptr || !ws || (node_capacity > 0 && !node_index) || (edge_capacity > 0 && (!senders || !receivers)))) {
        set_error("%s: null pointer argument", what);
        return GNF_EINVAL;
    }
    if (n_graphs == 0) return GNF_OK;   // an empty batch: nothing to write, no workspace to read
    const SubWs L = sub_ws(n_graphs, n_nodes, max_nodes_per_graph);
    if (ws_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, L.total);
        return GNF_EWORKSPACE;
    }
    if (!work || (node_capacity == 0 && edge_capacity == 0)) return GNF_OK;
    const char* base = (const char*)ws;
    hipLaunchKernelGGL(k_sub_fill, dim3(stats_grid((n_nodes + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const int32_t*)(base + L.off), n_graphs, n_nodes, max_nodes_per_graph, L.comp.stats.W,
                       (const unsigned long long*)(base + L.comp.stats.bitmap), (const int32_t*)(base + L.comp.stats.gid),
                       (const unsigned long long*)(base + L.keep), (const int32_t*)(base + L.rank),
                       (const int32_t*)(base + L.new_off), (const int32_t*)(base + L.new_id), (const int32_t*)(base + L.hdr),
                       rowptr, node_capacity, edge_capacity, node_index, senders, receivers);
    GNF_LAUNCH_CHECK("k_sub_fill");
    return GNF_OK;
}

}  // extern "C"
