/* include/gnf_adj_report.h - the reconstruction report entry points of libgnf_hip.so.  Included by gnf.h (which defines GnfCsr,
 * gnf_stream_t and the GNF_E* codes, includes gnf_distance.h for GnfDistance and opens the extern "C" block); not meant to be
 * included on its own. */
#ifndef GNF_ADJ_REPORT_H
#define GNF_ADJ_REPORT_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * WHICH node pairs do embeddings get wrong, and with what score: what run_gnn_inference.py:107-163 works out on the host from
 * the dense pred_adj and true adjacency of a test batch - pred_adj thresholded at 0.5 (:126-127), the pairs split into correct
 * edges, false positives and false negatives (:130-132), the quartiles of the scores of the two kinds of error (:133-144) and
 * per graph the "complete" graph with edge weights 1 / 2 / 3 and the predicted graph (:146-163) - on the device, without the
 * dense [n, n] blocks.
 *
 * Pair scores.  For graph g and an ordered pair (s, r), s != r, both in g:
 *   a_sr    = 1 when row r of the receiver-sorted CSR of the TRUE batch lists sender s.  Duplicate edges count once, self
 *             loops and senders from another graph are ignored: gnf_adj_loss.h's graph model.
 *   p_sr    the GnfDistance score: d2 the fp32 fmaf chain over the features in ascending order, u = temp * fmaf(-d2, scale,
 *             shift) with the product rounded on its own, p = 1 / (1 + expf(-u)) - the code gnf_pred_adj_dist_f32 evaluates, so
 *             p_sr has the bits of that entry point's block entry [r, s] (and of [s, r]: d2 is symmetric bit for bit).
 *   pred_sr = p_sr > threshold, the comparison gnf_adj_edges_count_dist_f32 makes.
 * Classes: 1 = a & pred (correct), 2 = !a & pred (false positive), 3 = a & !pred (false negative); a pair with neither is not
 * listed.  These are the weights of the reference's complete_mat (:153).
 *
 * Edge list.  Every pair with a | pred is one entry; receivers ascending, senders ascending within a receiver (the decoder's
 * order), so (rowptr, senders) is the receiver-sorted CSR of the list:
 *   senders, receivers  int32, batch-wide node ids        cls  int32, 1 / 2 / 3        score  fp32, p_sr
 *   rowptr int32 [n_nodes + 1]   n_edge int32 [n_graphs]   class_pairs int64 [n_graphs][3] (classes 1, 2, 3)
 *   totals int64 [4] = { entries, class 1, class 2, class 3 }
 * Consequences: the entries with cls in {1, 2} are exactly the edge list of gnf_adj_edges_count_dist_f32 /
 * gnf_adj_edges_fill without self loops at the same threshold, in order; the entries with cls in {1, 3} are the true batch's
 * deduplicated, loop-free, in-graph edges; class_pairs[g][1] / [2] are gnf_adj_loss_f32's fp_pairs / fn_pairs at threshold 0.5
 * and abs_tol 0.5.
 *
 * Two departures from the reference.  (1) Its pred_adj out of binary_loss keeps the diagonal, so run_gnn_inference.py counts
 * every node as a false-positive self loop with the score sigmoid(temp * shift); here the diagonal is excluded, as in loss.py's
 * own counts (loss.py:88-116).  (2) It drops scores that are exactly 0 from the false-negative quantiles (np.nonzero on the
 * masked matrix, :140-141); here they stay: a false negative at distance "infinity" is still a false negative.
 *
 * Route: gnf_adj_report_count_f32 builds the senders-into-row bitmap from the CSR (64-bit integer OR atomics), one workgroup
 * per (graph, 16-row tile) leaves one ballot word of pred per (row, 64 columns) beside the true word and the row's four
 * popcounts, the decoder's scan gives rowptr / n_edge / totals[0], two fixed-order integer reductions class_pairs and
 * totals[1..3].  gnf_adj_report_fill expands pred | true in the decoder's order and recomputes the score of the set bits with
 * the same chain.  Integers, ballots and comparisons only, no floating-point atomics: two calls give the same bytes.  dist->params
 * is read at run time by both.  Offsets that do not describe the batch (or a bound below the largest graph) give wrong
 * numbers, never an access outside the arrays.
 * ws: gnf_adj_report_workspace_bytes (a host computation), with W = ceil(max_nodes_per_graph / 64):
 *   node offsets int64 [n_graphs + 1]  |  true words uint64 [n_nodes][W]  |  pred words uint64 [n_nodes][W]  |
 *   row entry count int32 [n_nodes]  |  row class counts int32 [3][n_nodes]                      (rounded up to 8 bytes)
 * zeroed by a kernel; gnf_adj_report_fill reads what gnf_adj_report_count_f32 left there.
 * count: GNF_EINVAL: null csr / dist / rowptr / totals / z / ws / per-graph outputs / CSR arrays, missing node_offsets;
 * GNF_ESHAPE: D < 1, ld < D, negative sizes, max_nodes_per_graph < 0 or > 65536 (or 0 with nodes), n_nodes *
 * max_nodes_per_graph > INT32_MAX; GNF_EWORKSPACE: short workspace - all before any launch.  n_nodes == 0 or n_graphs == 0:
 * zeroed outputs, GNF_OK.  fill: the same rules on its own arguments, edge_capacity < 0 is GNF_ESHAPE; entries with an index
 * >= edge_capacity are dropped, nothing is written beyond it (totals still holds the full count).
 * Asynchronous on `stream`, nothing is read on the host, capturable. */
size_t gnf_adj_report_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph);
int gnf_adj_report_count_f32(const GnfCsr* csr, const GnfDistance* dist, const float* z, int64_t ld, int32_t D,
                             int32_t max_nodes_per_graph, float threshold,
                             int32_t* rowptr,        /* [n_nodes + 1] */
                             int32_t* n_edge,        /* [n_graphs] */
                             int64_t* class_pairs,   /* [n_graphs][3] */
                             int64_t* totals,        /* [4] */
                             void* ws, size_t ws_bytes, gnf_stream_t stream);
int gnf_adj_report_fill(const GnfDistance* dist, const float* z, int64_t ld, int32_t D, int64_t n_graphs, int64_t n_nodes,
                        int32_t max_nodes_per_graph, const int32_t* rowptr, int64_t edge_capacity, int32_t* senders,
                        int32_t* receivers, int32_t* cls, float* score, /* [edge_capacity] each */
                        const void* ws, size_t ws_bytes, gnf_stream_t stream);

/* Exact order statistics of the scores of one class, per segment of the edge list.  A segment is a run of nodes
 * [seg_nodes[s], seg_nodes[s + 1]) (cut to [0, n_nodes]) - { 0, n_nodes } for the whole batch, csr->node_offsets per graph -
 * and holds the entries [rowptr[first node], rowptr[last node + 1]) cut to [0, edge_capacity].  For class c in { 2, 3 }
 * (index 0, 1) take the segment's n scores of that class in ascending order x[0 .. n-1], and for every q[k] in [0, 1]:
 *   h = (n - 1) * q[k] (one fp64 product), lo = floor(h), hi = min(lo + 1, n - 1)
 *   stat[s][c][k] = { x[lo], x[hi] } fp32,  count[s][c] = n int64;  n == 0: both NaN.
 * The caller interpolates x[lo] + (h - lo) (x[hi] - x[lo]) in fp64 - np.quantile's linear rule (:137-138, :143-144) - so the device
 * does integers and selection only.  Order is that of the scores' bit patterns read as uint32: the numeric order of
 * non-negative floats, NaN last.  Selection is a radix select, four passes of 8 bits from the top, each a 256-bin histogram in
 * LDS with integer atomics and a scan of the bins; one workgroup per (segment, class, q); every loop is bounded by the
 * segment's entry count cut to the capacity.
 * GNF_EINVAL: null rowptr / seg_nodes, null stat / count with n_seg > 0, null score / cls with edge_capacity > 0, null q with
 * nq > 0;
 * GNF_ESHAPE: negative sizes, n_seg > INT32_MAX, nq > 16, a q outside [0, 1] (NaN included).  n_seg == 0: GNF_OK, nothing
 * written.  Asynchronous on `stream`, capturable (q is copied at the call). */
#define GNF_SELECT_MAX_Q 16
int gnf_score_select_f32(const float* score, const int32_t* cls, const int32_t* rowptr,
                         const int32_t* seg_nodes, /* device [n_seg + 1] */
                         int64_t n_seg, int64_t n_nodes, int64_t edge_capacity, const double* q /* host [nq] */, int32_t nq,
                         float* stat,    /* [n_seg][2][nq][2] */
                         int64_t* count, /* [n_seg][2] */
                         gnf_stream_t stream);

#endif /* GNF_ADJ_REPORT_H */
