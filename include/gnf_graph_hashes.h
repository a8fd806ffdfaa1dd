/* include/gnf_graph_hashes.h - the Weisfeiler-Lehman graph-hash and hash-matching entry points of libgnf_hip.so.  Included by
 * gnf.h (which defines GnfCsr, gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to be included on
 * its own. */
#ifndef GNF_GRAPH_HASHES_H
#define GNF_GRAPH_HASHES_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * Uniqueness and novelty of generated graphs - the share of generated graphs that repeat no earlier generated one, and the
 * share that repeat no training graph - on the device, beside the four distribution scores, which cannot see a sampler that
 * replays its training set.  Replaces nothing in the reference, which has no counterpart: it pickles the generated graphs
 * (generate_graphs.py:68-84).
 * Graph model and csr: exactly as gnf_graph_stats (undirected, simple: self loops ignored, duplicates once, one direction is
 * enough; csr->node_offsets / csr->n_graphs REQUIRED); the adjacency bitmap is gnf_graph_stats' (k_stats_bitmap).
 *
 * THE HASH (this definition, not the behaviour of any outside program, is what the tests hold the call to).  All arithmetic is
 * unsigned 64-bit, wrapping.
 *   mix(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;
 *            x ^= x >> 31
 *   KA = 0xA5A5A5A5A5A5A5A5, KB = 0xD6E8FEB86659FD93, KC = 0xFF51AFD7ED558CCD, KD = 0xC4CEB9FE1A85EC53
 * Per graph with n nodes and e simple undirected edges:
 *   c_i = mix(v_i), v_i the degree on the simple graph, or labels[i] (its 64 bits) when the caller passes labels
 *   h   = mix(n * 0x100000001B3 + e), then h = mix(h + sum_i mix(c_i ^ KA))
 *   for t = 1 .. iterations:  c'_i = mix(c_i * KC + sum_{j in N(i)} mix(c_j ^ KB) + t);  h = mix(h * KD + sum_i mix(c'_i ^ KA));
 *                             c = c'
 * A sum over no nodes is 0; the sums wrap, so their order does not matter: the result is bit-reproducible and the same under
 * any renumbering of a graph's nodes (labels permuted alike).
 * This is 1-dimensional Weisfeiler-Lehman colour refinement.  Isomorphic graphs get equal hashes; graphs that refinement
 * cannot separate collide BY DEFINITION - a 6-cycle against two triangles, any two regular graphs of equal size and degree.
 * `labels` is the way out: a node invariant that does separate them (the triangle column of gnf_graph_orbits for that pair).
 *
 * gnf_graph_hashes
 *   iterations         0 .. GNF_WL_MAX_ITERATIONS refinement rounds.
 *   labels             NULL, or device int64 [n_nodes]: the initial values v_i.
 *   hash[g]            uint64 [n_graphs]; a graph without nodes has the hash the definition gives for n = e = 0.
 *   node_colour[i]     uint64 [n_nodes]: c_i after the last round; 0 for a row that no graph covers or that lies past
 *                      max_nodes_per_graph inside its graph.
 *   n_edges[g]         int64 [n_graphs]: e.
 * Algorithm: the bitmap, then one of two routes, chosen on the host from max_nodes_per_graph; both give the same bits.
 *   <= GNF_WL_LDS_NODES: one launch, one workgroup per graph, both colour arrays in LDS (16 bytes per column), a wave per node
 *      row (lanes take the row's words and walk their set bits; rows of at most 256 columns: a lane per column), one workgroup
 *      barrier per round.
 *   above: the colours double-buffered in the workspace, one grid-stride launch per round with a wave per node, the per-graph
 *      sums by 64-bit integer atomics into a zeroed [iterations + 1][n_graphs] table, one small launch that folds it into h.
 * Cost per graph: the bitmap is read iterations + 1 times (n_g * ceil(max_nodes_per_graph / 64) * 8 bytes each), one mix per
 * directed edge and round.  Every loop is bounded by n_g, the words of a row, the 64 bits of a word or iterations: offsets or
 * edge lists that do not describe the batch give wrong numbers, never a hang or an access outside the arrays.
 * max_nodes_per_graph: any upper bound on n_node, at most GNF_WL_MAX_NODES (gnf_graph_stats' limit).
 * ws: gnf_graph_hashes_workspace_bytes (a host computation: the gnf_graph_stats workspace + two uint64 per node + the table
 * for GNF_WL_MAX_ITERATIONS rounds; 0 for arguments that no call accepts).
 * GNF_ESHAPE: max_nodes_per_graph < 0 or > GNF_WL_MAX_NODES (or 0 with nodes), iterations outside its range, negative sizes,
 * n_nodes or n_graphs above INT32_MAX; GNF_EINVAL: null pointers, missing node_offsets; GNF_EWORKSPACE: short workspace - all
 * before any launch.  n_graphs == 0: GNF_OK, nothing written.  n_nodes == 0: every graph gets the hash of the graph without
 * nodes, n_edges = 0.  Asynchronous on `stream`, no host synchronisation, no allocation, capturable. */
#define GNF_WL_MAX_ITERATIONS 64
#define GNF_WL_MAX_NODES 65536
#define GNF_WL_LDS_NODES 4096
size_t gnf_graph_hashes_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph);
int gnf_graph_hashes(const GnfCsr* csr, int32_t max_nodes_per_graph, int32_t iterations,
                     const int64_t* labels /* NULL or [n_nodes] */, uint64_t* hash /* [n_graphs] */,
                     uint64_t* node_colour /* [n_nodes] */, int64_t* n_edges /* [n_graphs] */,
                     void* ws, size_t ws_bytes, gnf_stream_t stream);

/* gnf_graph_hash_match: which graphs of a set A repeat an earlier graph of A, and which repeat a graph of a set B.  Two graphs
 * match when their hash AND their n_node are equal; a graph with n_node == 0 is left out (both indices -1, not counted).
 *   hash_a, n_node_a   uint64 [a], int32 [a] on the device;  hash_b, n_node_b likewise [b].  b == 0 is allowed (the pointers
 *                      may then be NULL): everything valid is novel.
 *   first_in_a[g]      int32 [a]: the smallest index in A with g's key - g itself exactly for the first of its kind.
 *   match_in_b[g]      int32 [a]: the smallest matching index in B, else -1.
 *   counts             int64 [4] = {valid, distinct (first_in_a[g] == g), novel (valid, no match in B), distinct and novel}.
 * One wave per graph of A: its lanes stride over A[0 .. g) and over B, then a wave minimum; the counts by integer atomics on
 * the zeroed array: two calls give the same bits.  Work: a (a / 2 + b) key comparisons.
 * ws: gnf_graph_hash_match_workspace_bytes (a host computation; one reserved 8-byte word, so that 0 still says "arguments that
 * no call accepts").
 * GNF_ESHAPE: a or b negative or above INT32_MAX; GNF_EINVAL: null pointers; GNF_EWORKSPACE: short workspace - all before any
 * launch.  a == 0: counts = {0, 0, 0, 0}, nothing else written.  Asynchronous on `stream`, no host synchronisation, no
 * allocation, capturable. */
size_t gnf_graph_hash_match_workspace_bytes(int64_t a, int64_t b);
int gnf_graph_hash_match(const uint64_t* hash_a, const int32_t* n_node_a, int64_t a,
                         const uint64_t* hash_b, const int32_t* n_node_b, int64_t b,
                         int32_t* first_in_a, int32_t* match_in_b /* [a] each */, int64_t* counts /* [4] */,
                         void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_GRAPH_HASHES_H */
