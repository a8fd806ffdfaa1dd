/* include/gnf_graph_components.h - the connected-component and subgraph-extraction entry points of libgnf_hip.so.  Included by
 * gnf.h (which defines GnfCsr, gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to be included on
 * its own. */
#ifndef GNF_GRAPH_COMPONENTS_H
#define GNF_GRAPH_COMPONENTS_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * Whether a generated graph is one graph at all, and the batch that is left when only some nodes are kept - the largest
 * connected component, the nodes with a neighbour, or a caller's mask - on the device, between the decoder (gnf_adj_edges_*)
 * and the scores (gnf_graph_stats, gnf_graph_orbits, gnf_graph_spectra).  Replaces nothing in the reference, which has no
 * counterpart: it pickles the generated graphs (generate_graphs.py:68-84).
 * Graph model and csr: exactly as gnf_graph_stats (undirected, simple: self loops ignored, duplicates once, one direction is
 * enough; csr->node_offsets / csr->n_graphs REQUIRED).  A row that no graph covers, or that lies past max_nodes_per_graph
 * inside its graph, belongs to no component and is never kept.  These definitions, not the behaviour of any outside program,
 * are what the tests hold the calls to.
 *
 * gnf_graph_components
 *   component[i]       int32 [n_nodes]: the batch-wide row of the smallest-index node of i's component (so component[r] == r
 *                      exactly for the roots) - canonical, independent of any search order; -1 for a row in no component.
 *   component_size[i]  int32 [n_nodes]: the number of nodes of that component; 0 for a row in no component.
 *   n_components[g]    int32 [n_graphs]: an isolated node is a component of size 1, a graph without nodes has 0.
 *   largest_size[g]    the size of the largest component, 0 for a graph without nodes.
 *   largest_root[g]    its root; among components of that size the smallest root; -1 for a graph without nodes.
 *   n_isolated[g]      the nodes of degree 0 on the simple graph.
 * Algorithm: the gnf_graph_stats bitmap, then one workgroup per graph: isolated nodes in one sweep, then breadth-first searches
 * from the smallest unlabelled node, level by level, on three bitsets (visited, frontier, next) of ceil(max_nodes_per_graph /
 * 64) words in LDS (<= 24 KiB).  Integer atomics only: two calls give the same bits.
 * Termination: every data-dependent loop is bounded by the graph's size n_g - at most n_g searches per graph, at most n_g
 * levels per search.  Offsets or edge lists that do not describe the batch give wrong labels, never a hang or an access
 * outside the arrays.
 * Cost per graph: the bitmap is read twice (n_g * ceil(max_nodes_per_graph / 64) * 8 bytes each: the isolated-node sweep, then
 * every row once when its node is on the frontier), and one pair of workgroup barriers per level - a path on n nodes costs up
 * to n levels, the price of a level-synchronous search (a 19 x 19 grid searched from a corner: 37).
 * max_nodes_per_graph: any upper bound on n_node, at most GNF_COMPONENTS_MAX_NODES (gnf_graph_stats' limit).
 * ws: gnf_graph_components_workspace_bytes (a host computation: the gnf_graph_stats workspace + 4 bytes per node; 0 for
 * arguments that no call accepts).
 * GNF_ESHAPE: max_nodes_per_graph < 0 or > GNF_COMPONENTS_MAX_NODES (or 0 with nodes), negative sizes, n_nodes or n_graphs
 * above INT32_MAX; GNF_EINVAL: null pointers, missing node_offsets; GNF_EWORKSPACE: short workspace - all before any launch.
 * n_graphs == 0: GNF_OK, nothing written.  n_nodes == 0: the per-graph outputs are zeroed, largest_root = -1.  Asynchronous
 * on `stream`, no host synchronisation, no allocation, capturable. */
#define GNF_COMPONENTS_MAX_NODES 65536
size_t gnf_graph_components_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph);
int gnf_graph_components(const GnfCsr* csr, int32_t max_nodes_per_graph,
                         int32_t* component, int32_t* component_size,                 /* [n_nodes] */
                         int32_t* n_components, int32_t* largest_size,
                         int32_t* largest_root, int32_t* n_isolated,                  /* [n_graphs] */
                         void* ws, size_t ws_bytes, gnf_stream_t stream);

/* gnf_graph_subgraph_count / gnf_graph_subgraph_fill: the subgraph of the simple undirected graph that a set of kept nodes
 * induces, as a new batch in the decoder's convention (gnf_adj_edges_*), in two calls like the decoder's: count, then - once the
 * caller knows N' and E' or has chosen capacities - fill.
 *   rule               GNF_KEEP_LARGEST_COMPONENT: component[i] == largest_root[g] (ties: the smallest root, as above);
 *                      GNF_KEEP_NON_ISOLATED: degree > 0;  GNF_KEEP_MASK: mask[i] != 0, mask a device uint8 [n_nodes] (ignored,
 *                      may be NULL, under the other rules).
 *   self_loops         0 / 1: with 1 every kept node also gets the edge (i, i); with 0 there is no diagonal at all.
 * The new batch keeps all n_graphs graphs (one with nothing kept has new_n_node = 0, so per-graph tensors of the old batch
 * still line up); kept nodes are renumbered in ascending old order, graph g's contiguous; both directions of every edge are
 * written, receivers ascending and senders ascending within a receiver - the loop at its sorted place.  The edge set is
 * symmetric, so (rowptr, senders) is the receiver-sorted CSR of the list and its by-sender transpose as well.
 *   new_id[i]          int32 [n_nodes]: the new batch-wide row of old row i, -1 for a row that is not kept.
 *   new_n_node, n_edge int32 [n_graphs] each.
 *   rowptr             int32 [n_nodes + 1] of room; the first N' + 1 entries are written.
 *   totals             int64 [2] = {N', E'}.
 *   node_index[r]      int32 [N']: the old row of new row r.       senders, receivers   int32 [E'] each.
 * fill reads the workspace that count left (the contract of gnf_adj_edges_fill: same sizes, same ws, nothing in between that
 * writes it) - the keep sets, the ranks and self_loops travel there.  Rows >= node_capacity and edges >= edge_capacity are
 * dropped, never written.  Vector stores only; every word has one writer: two calls give the same bits.
 * Limits: max_nodes_per_graph <= GNF_COMPONENTS_MAX_NODES and n_nodes * (max_nodes_per_graph + 1) <= INT32_MAX (the bound of
 * gnf_adj_edges_*, with room for the loops).
 * ws: gnf_graph_subgraph_workspace_bytes (a host computation; 0 for arguments that no call accepts), one size for both calls.
 * GNF_ESHAPE: the limits above, negative sizes or capacities, max_nodes_per_graph == 0 with nodes; GNF_EINVAL: null pointers,
 * missing node_offsets, an unknown rule, self_loops other than 0 / 1, GNF_KEEP_MASK with mask == NULL; GNF_EWORKSPACE: short
 * workspace - all before any launch.  n_graphs == 0: GNF_OK, nothing written.  n_nodes == 0: new_n_node and n_edge zeroed,
 * rowptr[0] = 0, totals = {0, 0}.  Asynchronous on `stream`, no host synchronisation, no allocation, capturable. */
#define GNF_KEEP_LARGEST_COMPONENT 0
#define GNF_KEEP_NON_ISOLATED 1
#define GNF_KEEP_MASK 2
size_t gnf_graph_subgraph_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph);
int gnf_graph_subgraph_count(const GnfCsr* csr, int32_t max_nodes_per_graph, int32_t rule, const uint8_t* mask,
                             int32_t self_loops, int32_t* new_id, int32_t* new_n_node,
                             int32_t* rowptr /* [n_nodes + 1], first N' + 1 valid */, int32_t* n_edge,
                             int64_t* totals /* [2] */, void* ws, size_t ws_bytes, gnf_stream_t stream);
int gnf_graph_subgraph_fill(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph, const int32_t* rowptr,
                            int64_t node_capacity, int64_t edge_capacity, int32_t* node_index,
                            int32_t* senders, int32_t* receivers, void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_GRAPH_COMPONENTS_H */
