/* include/gnf_adj_loss.h - the adjacency reconstruction loss entry points of libgnf_hip.so.  Included by gnf.h (which defines
 * GnfCsr, gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to be included on its own. */
#ifndef GNF_ADJ_LOSS_H
#define GNF_ADJ_LOSS_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * How well do embeddings reconstruct the graph they belong to: binary_loss (loss.py:162-188), the edge-error counts
 * (loss.py:88-116) and the gradient of that loss with respect to the embeddings (what tf.gradients gives run_gnn.py), on the
 * device and without the dense [N, N] matrices the reference builds (true_adj, pred_adj, ce_loss are not produced).
 *
 * The distance function: p_ij = sigmoid(u_ij), u_ij = temp * (shift - d2_ij * scale), d2_ij the fp32 fmaf chain over the
 * features in ascending order of (z_i[f] - z_j[f])^2 and scale = 1 / sqrtf((float)D) (scale_by_sqrt_dim != 0) or 1 -
 * evaluated by the code gnf_pred_adj_f32 evaluates it with (u = temp * fmaf(-d2, scale, shift), the product rounded on its
 * own), so for temp = 10, shift = 1, scale_by_sqrt_dim = 1 p_ij has the bits of gnf_pred_adj_f32's block entry and of the
 * value gnf_adj_edges_count_f32 thresholds.  This entry point is gnf_adj_loss_dist_f32 (gnf_distance.h) with the distance
 * taken from spec, without grad_params and without the tail of that entry point's workspace.
 *   scaled_hacky_sigmoid_l2 (loss.py:45-53): 10, 1, on;  hacky_sigmoid_l2 (loss.py:36-42): 10, 1, off;
 *   sigmoid_l2(temp, shift) (loss.py:56-62): temp, shift, on.  The other distance functions of loss.py are not covered. */
typedef struct GnfAdjLossSpec {
    float temp, shift;
    int32_t scale_by_sqrt_dim; /* 0: scale = 1 */
    int32_t soft_labels;       /* 0: t = a;  else t = 1 - label_epsilon where a = 1, label_epsilon where a = 0 (loss.py:173-176) */
    float label_epsilon;       /* in [0, 0.5] */
    float abs_tol;             /* >= 0: the counts' threshold (loss.py's abs_tol, 0.5 there) */
} GnfAdjLossSpec;

/* Graph model.  csr is the receiver-sorted CSR of the TRUE batch (gnf_build_csr, or the one gnf_adj_edges_* produce);
 * csr->node_offsets / csr->n_graphs are REQUIRED.  The graph is read as DIRECTED: for an ordered pair (i, j), i != j, both
 * in graph g, a_ij = 1 when CSR row j (receiver j) lists sender i - true_adj[i, j] of loss.py:66-70 - and 0 otherwise.
 * Duplicate edges count once (the reference's einsum counts their multiplicity; the datasets hold none); self loops and
 * edges whose sender lies in another graph are ignored (the reference's mask and remove_diag drop them as well).
 *   counts   in fp32 against the hard label: fp_pairs[g] = ordered pairs of g with p - a > abs_tol, fn_pairs[g] = those with
 *            a - p > abs_tol, int64 [n_graphs] (the reference's edge figures are these halved, loss.py:95,101: host side)
 *   loss     ce_ij = softplus(u_c) - t_ij u_c, u_c = clamp(u_ij, -U, U), U = log((1 - 1e-7) / 1e-7): in exact arithmetic
 *            tf.keras.backend.binary_crossentropy of TF 1.x (probability clipped to [1e-7, 1 - 1e-7], logit, sigmoid
 *            cross-entropy with logits; 1e-7 is Keras' epsilon).  Evaluated as max(u, 0) + log1pf(expf(-|u|)) - t u, the terms
 *            added in fp64; loss_per_graph[g] = sum over the ordered pairs of g, fp64 [n_graphs];
 *            sums2[0] = sum_g loss_per_graph[g], sums2[1] = sums2[0] / (N^2 - N), N = csr->n_nodes (loss.py:186-187; 0 for
 *            N < 2), fp64 [2]
 *   grad     NULL, or fp32 [n_nodes][ld_grad], columns 0..D-1 written (every row: zeros where no graph covers it):
 *            grad_i = grad_scale * sum_{j != i} c_ij (z_i - z_j), c_ij = -2 temp scale ((p_ij - t_ij) + (p_ij - t_ji)) where
 *            |u_ij| < U and 0 where the clip is active (tf.clip_by_value passes no gradient there: a true edge whose
 *            endpoints lie far apart gets none).  grad_scale = 1 differentiates sums2[0], 1 / (N^2 - N) sums2[1].
 * No floating-point atomics and fixed-order reductions: every row is owned by one workgroup, row sums (fp64 / int32) go to
 * the workspace, one wave per graph adds its rows up, one wave the graphs - two calls on the same input give the same bits.
 * max_nodes_per_graph: any upper bound on n_node, at most 65536.  A graph larger than the bound is the caller's error:
 * its surplus rows are dropped.  Offsets that do not describe the batch give wrong numbers, never an access outside the
 * arrays.
 * ws: gnf_adj_loss_workspace_bytes (a host computation): with W = ceil(max_nodes_per_graph / 64),
 *   senders into row i   uint64 [n_nodes][W]  (bit j - n0: a_ji)  |  receivers out of row i  uint64 [n_nodes][W]  (a_ij)  |
 *   row loss fp64 [n_nodes]  |  row fp count int32 [n_nodes]  |  row fn count int32 [n_nodes]      (rounded up to 8 bytes)
 * zeroed by a kernel (a memset node of a replayed capture is not reliably ordered before the kernels behind it).
 * GNF_EINVAL: null pointers (csr, spec, sums2, z, ws, the per-graph outputs, the CSR arrays), missing node_offsets;
 * GNF_ESHAPE: D < 1, ld < D, ld_grad < D (with grad), negative sizes, max_nodes_per_graph < 0 or > 65536 (or 0 with nodes),
 * label_epsilon outside [0, 0.5], abs_tol < 0; GNF_EWORKSPACE: short workspace - all before any launch.
 * n_nodes == 0 or n_graphs == 0: the outputs are zeroed, GNF_OK.  Asynchronous on `stream`, no host synchronisation,
 * capturable. */
size_t gnf_adj_loss_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph);
int gnf_adj_loss_f32(const GnfCsr* csr, const float* z, int64_t ld, int32_t D, int32_t max_nodes_per_graph,
                     const GnfAdjLossSpec* spec,
                     double* loss_per_graph,                 /* [n_graphs] */
                     double* sums2,                          /* [2]: sum loss, mean loss */
                     int64_t* fp_pairs, int64_t* fn_pairs,   /* [n_graphs] */
                     float* grad, int64_t ld_grad, float grad_scale, /* [n_nodes][ld_grad] or NULL */
                     void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_ADJ_LOSS_H */
