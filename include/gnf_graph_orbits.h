/* include/gnf_graph_orbits.h - the orbit-count entry points of libgnf_hip.so.  Included by gnf.h (which defines GnfCsr,
 * gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to be included on its own. */
#ifndef GNF_GRAPH_ORBITS_H
#define GNF_GRAPH_ORBITS_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * The third statistic of GraphRNN-style evaluation, on the device: the 15 node orbits of the graphlets on 2, 3 and 4 nodes
 * and the MMD of per-graph mean orbit vectors.  Replaces nothing in the reference, which has no counterpart: it pickles the
 * generated graphs (generate_graphs.py:68-84) and leaves orbit counting to an outside program run on host edge lists.
 * Graph model and csr: exactly as gnf_graph_stats (undirected, simple; csr->node_offsets / csr->n_graphs REQUIRED).
 *   orbits[v][o]      int64 [n_nodes][ld_orbits], columns 0..14 written: the number of INDUCED connected subgraphs on 2, 3 or
 *                     4 nodes that contain node v, with v in automorphism orbit o - Przulj's numbering (the one ORCA uses):
 *                       0 edge | 1 path3 end | 2 path3 middle | 3 triangle | 4 path4 end | 5 path4 inner | 6 star leaf |
 *                       7 star centre | 8 4-cycle | 9 tailed triangle, tail end | 10 tailed triangle, triangle node of degree 2 |
 *                       11 tailed triangle, node of degree 3 | 12 chorded 4-cycle, degree 2 | 13 chorded 4-cycle, degree 3 | 14 K4
 *                     (orbits[v][0] = degree, orbits[v][3] = triangles of gnf_graph_stats).  A row that no graph covers, or
 *                     that lies past max_nodes_per_graph inside its graph, gets zeros.
 *   orbit_sums[g][o]  int64 [n_graphs][15]: sum of orbits[v][o] over the nodes of graph g (zeroed by the call, then 64-bit
 *                     integer atomics: deterministic).  A graph's orbit vector is orbit_sums[g] / n_node[g] in fp64.
 * Exact 64-bit integer arithmetic throughout.  max_nodes_per_graph: any upper bound on n_node, at most 8192 (the cost per
 * node is (n_g + d_i d_mean) ceil(max_nodes_per_graph / 64) word operations).  ws: gnf_graph_orbits_workspace_bytes (a host
 * computation: the gnf_graph_stats bitmap and three int32 per node).
 * GNF_ESHAPE: max_nodes_per_graph < 0 or > 8192 (or 0 with nodes), ld_orbits < 15, negative sizes; GNF_EINVAL: null
 * pointers, missing node_offsets; GNF_EWORKSPACE: short workspace - all before any launch.  n_graphs == 0: GNF_OK, nothing
 * written.  Asynchronous on `stream`, no host synchronisation, capturable. */
size_t gnf_graph_orbits_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph);
int gnf_graph_orbits(const GnfCsr* csr, int32_t max_nodes_per_graph,
                     int64_t* orbits, int64_t ld_orbits,      /* [n_nodes][ld_orbits], ld_orbits >= 15 */
                     int64_t* orbit_sums,                     /* [n_graphs][15] */
                     void* ws, size_t ws_bytes, gnf_stream_t stream);
/* MMD block sums of two sets of vectors given as int64 sums A [a][L] (row stride lda), B [b][L] (row stride ldb) and int32
 * counts: row r stands for xa[r][:] / count_a[r] in fp64 (orbit_sums / n_node); rows with count <= 0 (a graph without nodes)
 * are excluded.  k(x, y) = exp(-|x - y|_2^2 / (2 sigma^2)) on the raw vectors (no normalisation to a pmf); GraphRNN's orbit
 * setting is sigma = 30.  out5 as gnf_hist_mmd_f64: { sum AA, sum BB, sum AB, cnt_a, cnt_b }, diagonals included.  Replaces
 * nothing in the reference (no counterpart, as above).  No floating-point atomics, a fixed-order reduction: two calls give
 * the same bits, and two identical sets give sum AA == sum BB == sum AB bit for bit.  ws: gnf_vec_mmd_workspace_bytes(a, b)
 * (host computation).  GNF_ESHAPE: negative sizes, L > lda, L > ldb; GNF_EINVAL: sigma <= 0, null pointers; GNF_EWORKSPACE
 * - all before any launch.  a + b == 0: five zeros. */
size_t gnf_vec_mmd_workspace_bytes(int64_t a, int64_t b);
int gnf_vec_mmd_i64(const int64_t* xa, const int32_t* count_a, int64_t a, int64_t lda,
                    const int64_t* xb, const int32_t* count_b, int64_t b, int64_t ldb,
                    int32_t L, double sigma, double* out5, void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_GRAPH_ORBITS_H */
