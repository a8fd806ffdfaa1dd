/* include/gnf_graph_spectra.h - the Laplacian-spectrum entry points of libgnf_hip.so.  Included by gnf.h (which defines
 * GnfCsr, gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to be included on its own. */
#ifndef GNF_GRAPH_SPECTRA_H
#define GNF_GRAPH_SPECTRA_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * The fourth statistic of graph-generation evaluation (reported since GRAN), on the device: the eigenvalues of every graph's
 * normalised Laplacian and their per-graph histogram, whose MMD gnf_hist_mmd_f64 (GNF_MMD_GAUSSIAN_TV) computes.  Replaces
 * nothing in the reference, which has no counterpart: it pickles the generated graphs (generate_graphs.py:68-84).
 * Graph model and csr: exactly as gnf_graph_stats (undirected, simple: self loops ignored, duplicates once, one direction is
 * enough; csr->node_offsets / csr->n_graphs REQUIRED).
 *   Matrix, with d_i the degree on that simple graph:  L_ii = 1 if d_i > 0 else 0;  L_ij = -1 / sqrt(d_i d_j) for an edge,
 *                     else 0 - an isolated node contributes an eigenvalue 0 (DH (D - A) DH with DH_ii = 0 there).
 *   eigenvalues       double [n_nodes]: graph g's n_g eigenvalues in ascending order in eigenvalues[node_offsets[g] ..
 *                     node_offsets[g+1]).  A row that no graph covers, or that lies past max_nodes_per_graph inside its
 *                     graph, gets 0.
 *   hist[g][b]        int32 [n_graphs][bins] (NULL with bins == 0: no histogram): every eigenvalue x of graph g adds one count
 *                     to bin  b = clamp(floor((x - lo) * bins / (hi - lo)), 0, bins - 1)  evaluated in fp64 in that order.
 *                     The clamp IS the definition: values outside [lo, hi) land in the first / last bin (the top eigenvalue
 *                     of a bipartite component is 2 up to rounding, on either side).  This definition, not the behaviour of
 *                     any outside program, is what the tests hold the call to; lo = -1e-5, hi = 2, bins = 200 is the
 *                     Python layer's default.  The call writes the whole row: it sums to n_g, all zeros for a graph
 *                     without nodes.
 * All arithmetic is fp64: Householder tridiagonalisation, then bisection on Sturm counts with a fixed number of halvings;
 * fixed-order reductions and integer atomics only, so two calls give the same bits.
 * max_nodes_per_graph: any upper bound on n_node, at most GNF_SPECTRA_MAX_NODES.  Up to GNF_SPECTRA_LDS_NODES a graph's
 * matrix lives in LDS: 8 n^2 (matrix) + 32 n (four vectors) + 4224 (reduction scratch, histogram chunk) bytes <= 160 KiB
 * gives n <= 139.  Above it the matrix lives in the workspace, in min(n_graphs, GNF_SPECTRA_SLOTS) slots of
 * max_nodes_per_graph^2 doubles; workgroup w takes graphs w, w + GNF_SPECTRA_SLOTS, ...
 * ws: gnf_graph_spectra_workspace_bytes (a host computation: the gnf_graph_stats bitmap, then the slots if any; 0 for
 * arguments that no call accepts).
 * GNF_ESHAPE: max_nodes_per_graph < 0 or > GNF_SPECTRA_MAX_NODES (or 0 with nodes), bins < 0, bins > 0 with hi <= lo (or a
 * NaN), negative sizes; GNF_EINVAL: null pointers, missing node_offsets, hist == NULL with bins > 0; GNF_EWORKSPACE: short
 * workspace - all before any launch.  n_graphs == 0: GNF_OK, nothing written.  Asynchronous on `stream`, no host
 * synchronisation, no allocation, capturable. */
#define GNF_SPECTRA_MAX_NODES 2048
#define GNF_SPECTRA_LDS_NODES 139
#define GNF_SPECTRA_SLOTS 256
size_t gnf_graph_spectra_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph);
int gnf_graph_spectra(const GnfCsr* csr, int32_t max_nodes_per_graph,
                      double* eigenvalues,            /* [n_nodes] */
                      int32_t* hist, int32_t bins,    /* [n_graphs][bins], nullable with bins == 0 */
                      double lo, double hi,
                      void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_GRAPH_SPECTRA_H */
