/* include/gnf_random_graphs.h - random graph models generated on the device as edge lists in the decoder's order, with both
 * CSRs: G(n, p) and the planted partition model, and Barabasi-Albert preferential attachment.  They are the baseline rows of
 * the graph scores (GraphRNN-style tables put Erdos-Renyi and Barabasi-Albert beside the model) and a source of graph batches
 * of chosen size and density that needs no data file.
 * Included by gnf.h (which defines gnf_stream_t and the GNF_E* codes and opens the extern "C" block) after gnf_synthetic.h (for
 * gnf_syn_draw); not meant to be included on its own. */
#ifndef GNF_RANDOM_GRAPHS_H
#define GNF_RANDOM_GRAPHS_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * The reference has no counterpart (graph_data.py only loads pickled graphs), so everything here is a DEFINITION, as
 * gnf_perturb.h's and gnf_synthetic.h's randomness is: integers only, no floating point anywhere in the library part, so that
 * the device, the numpy twin (random_graphs.random_graphs_host) and a pure-Python restatement agree integer for integer.
 *
 * CONVENTIONS OF BOTH MODELS.  Graph b of the call has n = n_node[b] nodes with local ids 0 .. n - 1 and the draw index
 * G = first_graph + b: graphs 0 .. B - 1 from one call are the graphs of two calls of B / 2 with first_graph = 0 and B / 2.
 * The seed is the host value `seed`, or - seed_dev != NULL - the word the kernels read from the device at run time (as
 * GnfPerturbSpec does it); the kernels never write it.  The result is a simple undirected graph stored as both directed
 * edges; self_loops != 0 adds one loop per node (the datasets' convention, graph_data.py:43).  Edge order is the decoder's
 * (gnf_adj_edges_fill): receivers ascend, senders ascend within a receiver, batch-wide node ids - hence (rowptr, senders) is
 * the by-receiver CSR and, the edge set being symmetric, its by-sender transpose as well.
 *
 * GNF_RG_PLANTED (planted partition; Erdos-Renyi G(n, p) is the one-block case).  The pair lo < hi is an edge iff
 *   gnf_syn_draw(seed, G, lo, hi) < thr                                   (a 32-bit draw against a uint64 threshold)
 * with thr = thr_in[b] when block(lo) == block(hi), else thr_out[b]; thr_out == NULL means thr_in everywhere: G(n, p).
 * thr_in / thr_out are device uint64 [B], read at run time; the caller computes thr = (uint64)(p * 4294967296.0), an exact
 * product: 2^32 (or anything above) takes every pair, 0 takes none.  `block` is a device int32 [N] of block labels per node
 * (batch-wide node index; labels are only compared, never used as an index); block == NULL means
 * block(i) = (i * n_blocks) / n in 64-bit arithmetic, n_blocks >= 1 a host value: contiguous blocks of near-equal size.
 *
 * GNF_RG_BARABASI_ALBERT, with m = clamp(m_dev[b], 1, max_m); m_dev is a device int32 [B], max_m <= GNF_RG_MAX_M a host
 * bound.  Nodes 0 .. m - 1 start without edges; node t = m attaches to all of 0 .. m - 1; node t > m attaches to m distinct
 * earlier nodes drawn by degree.  Let R_t be the concatenation over t' = m .. t - 1 of (targets(t')[0 .. m - 1], then t'
 * repeated m times): |R_t| = 2 m (t - m), every node appears in it once per edge end it holds, and R_t[k] needs only the
 * targets table: t' = m + k / 2m, c = k % 2m; c < m gives targets(t')[c], else t'.
 *   for j = 0, 1, .. < GNF_RG_BA_DRAWS:  k_j = (gnf_syn_draw(seed ^ 0xA5A5A5A5A5A5A5A5, G, t, j) * |R_t|) >> 32
 *   candidate R_t[k_j] is accepted iff it differs from every candidate accepted before for this t
 *   targets(t) = the first m accepted, in order of j
 * If fewer than m were accepted after the GNF_RG_BA_DRAWS draws, the rest are the smallest-numbered nodes < t not yet accepted
 * (there are always enough: t > m).  n <= m gives no edges.  Every loop is bounded by n, m or GNF_RG_BA_DRAWS.  For n > m the
 * graph has exactly m (n - m) undirected edges, every node t >= m has degree >= m, and the graph is connected.
 * (A candidate is accepted iff it is the FIRST occurrence of its value among the draws of t - the form the kernel evaluates:
 * lane j evaluates draw j, first occurrences by an LDS integer max, ranks by ballot and prefix popcount.)
 * With (n, m) = (200, 16), (130, 8), (65, 4) no node needs more than 104 draws; the fallback is met only when m is close
 * to n, e.g. (44, 40) and (70, 64), where the distinct nodes of R_t are barely m.
 *
 * LIMITS.  The targets table ((n - m) m entries) of a graph sits in LDS beside one int32 per node:
 *   max_nodes_per_graph * max_m <= GNF_RG_BA_TABLE_MAX (32768 entries, 128 KB) and
 *   4 * (max_nodes_per_graph * (max_m + 1) + 4) bytes <= 160 KB (the LDS of a gfx950 compute unit);
 * beyond either, GNF_EUNSUPPORTED before any launch. */
enum { GNF_RG_PLANTED = 0, GNF_RG_BARABASI_ALBERT = 1 };
#define GNF_RG_BA_DRAWS 256
#define GNF_RG_MAX_M 64
#define GNF_RG_BA_TABLE_MAX 32768
#define GNF_RG_BA_SEED_XOR 0xA5A5A5A5A5A5A5A5ull

typedef struct GnfRandomGraphSpec {
    uint64_t seed;            /* read without seed_dev */
    const uint64_t* seed_dev; /* NULL, or one device word read at run time */
    uint64_t first_graph;     /* draw index of graph 0 of the call */
    int32_t model;            /* GNF_RG_PLANTED / GNF_RG_BARABASI_ALBERT */
    int32_t self_loops;       /* != 0: one loop per node */
    const uint64_t* thr_in;   /* planted: device uint64 [B] */
    const uint64_t* thr_out;  /* planted: device uint64 [B], or NULL = thr_in */
    const int32_t* block;     /* planted: device int32 [N] block labels, or NULL = n_blocks contiguous blocks */
    int32_t n_blocks;         /* planted with block == NULL: >= 1 */
    int32_t max_m;            /* Barabasi-Albert: 1 .. GNF_RG_MAX_M */
    const int32_t* m_dev;     /* Barabasi-Albert: device int32 [B] */
} GnfRandomGraphSpec;

/* gnf_random_graph_edges_count: pass 1 of the edge list.  The arguments after `spec` are gnf_adj_edges_count_f32's: n_node
 * device int32 [B], n_nodes = N, max_nodes_per_graph the caller's bound on n_b (a larger graph is cut to it); rowptr [N + 1],
 * n_edge [B], total [1] (device).  ws: gnf_adj_edges_workspace_bytes(n_graphs, n_nodes, max_nodes_per_graph).  The call leaves
 * the 64-bit adjacency bitmap and the row counts in the workspace in exactly the layout gnf_adj_edges_fill reads and runs the
 * decoder's scan; gnf_adj_edges_fill with the same sizes and workspace then writes senders / receivers and honours
 * edge_capacity.
 *   planted: the decoder's grid and row ownership - one workgroup per (graph, 16-row tile), lane = column, one ballot per row
 *     and 64 columns = one bitmap word, popcounts summed in registers; (i, j) and (j, i) evaluate the same function, so the
 *     bitmap is symmetric by construction.  No atomics.  Cost: one hash round per ordered pair (the graph's round is done once per workgroup, the
 *     lower node's once per row and per column of a wave).
 *   Barabasi-Albert: the workspace's bitmap and row counts are zeroed by a stream-ordered memset, then one workgroup of
 *     GNF_RG_BA_DRAWS lanes per graph walks t = m .. n - 1 (three barriers per node) with the targets table in dynamic LDS,
 *     sets the bits with 64-bit integer OR atomics - which commute: the result is deterministic - and counts degrees in LDS.
 * Every index derived from n_node, block or m_dev is clamped: wrong counts lose edges, never leave the arrays.  No float
 * atomics, no floating point: two calls give the same bits.
 * GNF_EINVAL: null spec, rowptr, total or ws, null n_node / n_edge with graphs, missing thr_in (planted) or m_dev (Barabasi-
 * Albert), unknown model; GNF_ESHAPE: negative sizes, n_graphs above INT32_MAX, n_blocks < 1 with block == NULL, max_m outside
 * 1 .. GNF_RG_MAX_M, the decoder's size rules (max_nodes_per_graph == 0 with nodes, n_nodes * max_nodes_per_graph above
 * INT32_MAX); GNF_EWORKSPACE: short workspace; GNF_EUNSUPPORTED: LIMITS above - all before any launch, gnf_last_error() starts
 * with the function's name.  n_graphs == 0 or n_nodes == 0: GNF_OK with rowptr[0] = 0 and *total = 0 (n_edge = 0 for every
 * graph there is).
 * Asynchronous on `stream`, no host synchronisation, no allocation, capturable (the spec's host values are fixed at capture;
 * seed_dev, thr_in, thr_out, block, m_dev and n_node are read at run time). */
int gnf_random_graph_edges_count(const GnfRandomGraphSpec* spec, const int32_t* n_node, int64_t n_graphs, int64_t n_nodes,
                                 int32_t max_nodes_per_graph, int32_t* rowptr, int32_t* n_edge, int64_t* total, void* ws,
                                 size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_RANDOM_GRAPHS_H */
