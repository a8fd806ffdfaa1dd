/* include/gnf_distance.h - one distance-function description for the adjacency loss, the dense decoder and the edge-list
 * decoder of libgnf_hip.so, with parameters that may live on the device.  Included by gnf.h (which defines GnfCsr,
 * gnf_stream_t and the GNF_E* codes, opens the extern "C" block and includes gnf_adj_loss.h first); not meant to be included
 * on its own. */
#ifndef GNF_DISTANCE_H
#define GNF_DISTANCE_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * run_gnn.py chooses the decoder's distance function with --binary_dist_fn and, with --tune_sigmoid, makes temp and shift of
 * sigmoid_l2 trainable variables (run_gnn.py:146-165).  The entry points below take the distance function as an argument -
 * p_ij = sigmoid(u_ij), u_ij = temp * (shift - d2_ij * scale), the arithmetic gnf_adj_loss.h documents, spelled out as
 * u = temp * fmaf(-d2, scale, shift) with the product rounded on its own: the three of them give the same bits for the same
 * (temp, shift, scale).  gnf_pred_adj_f32, gnf_adj_edges_count_f32 and gnf_adj_loss_f32 are the same code paths with
 * {10, 1, 1, NULL}, {10, 1, 1, NULL} and spec's {temp, shift, scale_by_sqrt_dim, NULL}: the same kernels, the same bits.
 *   scaled_hacky_sigmoid_l2: {10, 1, 1, NULL};  hacky_sigmoid_l2: {10, 1, 0, NULL};  sigmoid_l2(temp, shift): {temp, shift, 1,
 *   NULL};  trainable: params = device {temp, shift}, which every workgroup of the pair kernels loads once, at run time, with
 *   an ordinary load - nothing of them is read on the host or passed by value. */
typedef struct GnfDistance {
    float temp, shift;          /* used when params == NULL */
    int32_t scale_by_sqrt_dim;  /* 0: scale = 1, else 1 / sqrtf((float)D) */
    const float* params;        /* NULL, or DEVICE fp32 [2] = {temp, shift}: read by the kernels at run time */
} GnfDistance;

/* gnf_pred_adj_f32 under `dist`: the remaining arguments, the checks, the error codes and the workspace
 * (gnf_pred_adj_workspace_bytes) are that entry point's.  GNF_EINVAL for a null dist. */
int gnf_pred_adj_dist_f32(const GnfDistance* dist, const float* z, int64_t ld, int32_t D, const int32_t* n_node,
                          int64_t n_graphs, int32_t max_nodes_per_graph, float* out_blocks, int64_t* block_off, void* ws,
                          size_t ws_bytes, gnf_stream_t stream);

/* gnf_adj_edges_count_f32 under `dist`: likewise (gnf_adj_edges_workspace_bytes); gnf_adj_edges_fill follows it unchanged.
 * GNF_EINVAL for a null dist. */
int gnf_adj_edges_count_dist_f32(const GnfDistance* dist, const float* z, int64_t ld, int32_t D, const int32_t* n_node,
                                 int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph, float threshold,
                                 int32_t self_loops, int32_t* rowptr, int32_t* n_edge, int64_t* total, void* ws, size_t ws_bytes,
                                 gnf_stream_t stream);

/* gnf_adj_loss_f32 under `dist`, which overrides spec->temp, spec->shift and spec->scale_by_sqrt_dim, and the gradient of the
 * summed loss with respect to the two parameters:
 *   grad_params  NULL, or device fp32 [2] = grad_scale * {dL/dtemp, dL/dshift}.  With w_ij = shift - d2_ij * scale, over the
 *                ordered pairs i != j of every graph with |u_ij| < U (tf.clip_by_value passes no gradient where it clips: the
 *                rule the node gradient follows),
 *                  dL/dtemp = sum (p_ij - t_ij) w_ij          dL/dshift = temp sum (p_ij - t_ij)
 *                Each term is formed in fp32 operands and added in fp64 per row beside the row loss (the sum of p_ij - t_ij
 *                without the factor temp); the rows are added up per graph and the graphs in the fixed order of the loss, the
 *                factor temp is applied in fp64 and the result is rounded to fp32 once.  No floating-point atomics: two
 *                calls on the same input give the same bits.  The other outputs have the bits gnf_adj_loss_f32 gives for
 *                the same (temp, shift, scale).
 * ws: gnf_adj_loss_dist_workspace_bytes (a host computation): gnf_adj_loss_f32's layout, then, from its (8-byte rounded) end,
 *   row dtemp fp64 [n_nodes]  |  row dshift fp64 [n_nodes]  |  graph dtemp fp64 [n_graphs]  |  graph dshift fp64 [n_graphs]
 * (the tail is touched with grad_params only).  Checks and codes are gnf_adj_loss_f32's, plus GNF_EINVAL for a null dist.  n_nodes == 0 or n_graphs == 0: the outputs,
 * grad_params included, are zeroed.  Asynchronous on `stream`, nothing is read from the host after launch, capturable. */
size_t gnf_adj_loss_dist_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t max_nodes_per_graph);
int gnf_adj_loss_dist_f32(const GnfCsr* csr, const float* z, int64_t ld, int32_t D, int32_t max_nodes_per_graph,
                          const GnfAdjLossSpec* spec, const GnfDistance* dist,
                          double* loss_per_graph,                 /* [n_graphs] */
                          double* sums2,                          /* [2]: sum loss, mean loss */
                          int64_t* fp_pairs, int64_t* fn_pairs,   /* [n_graphs] */
                          float* grad, int64_t ld_grad, float grad_scale, /* [n_nodes][ld_grad] or NULL */
                          float* grad_params,                     /* [2] or NULL */
                          void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_DISTANCE_H */
