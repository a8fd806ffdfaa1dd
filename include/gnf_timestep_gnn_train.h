/* include/gnf_timestep_gnn_train.h - training the encoder: TimestepGNN's forward pass with a stash, and its backward pass
 * (what optimizer.compute_gradients walks through at run_gnn.py:270-296).  Included by gnf.h behind gnf_timestep_gnn.h (which
 * defines GnfTimestepGnn, GnfSntBatchNorm and GnfRowNorm); not meant to be included on its own. */
#ifndef GNF_TIMESTEP_GNN_TRAIN_H
#define GNF_TIMESTEP_GNN_TRAIN_H
#ifndef GNF_TIMESTEP_GNN_H
#error "include gnf.h, which includes gnf_timestep_gnn.h and then this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 *
 * Both entry points take message-passing nets only (sum or mean aggregator, agg or concat combine): a net with an attention
 * front-end (edge-list or graph scope) is GNF_EUNSUPPORTED from both, before any launch.
 *
 * ---- training forward --------------------------------------------------------------------------------------------------
 * gnf_timestep_gnn_train_forward_f32 computes exactly what gnf_timestep_gnn_f32 computes with is_training = 1 - out, the
 * batch moments and the moving-average update, bit for bit: the launches are the same, only their destinations differ -
 * and leaves in `stash` what the backward pass needs and cannot recompute cheaply.  The stash holds O(T N D) floats and no
 * hidden activation of any MLP (the backward recomputes those):
 *     in[i]   fp32 [n_nodes][D], i = 1 .. T-1   the rows that entered timestep i (= the module's output of timestep i-1,
 *                                                written there directly; timestep 0's rows are the caller's x)
 *     v[i]    fp32 [n_nodes][D], i = 0 .. T-1   with bns or lns only: the rows that entered GNN_i (the norm stage's output,
 *                                                written there directly); without norms v[i] is in[i]
 *     mean[i], var[i]   fp32 [D] each, i = 0 .. T-1, with bns only: the batch moments that normalised timestep i.  The
 *                                                stash always keeps them; bns[i].batch_mean / batch_variance, where not
 *                                                NULL, receive a copy.
 * Every region's offset from the stash's base is a multiple of 256 bytes (the base itself needs 8-byte alignment only).  The
 * stash belongs to one (csr, g, x) call: the backward pass must be given the same csr, g, x and D.  g->is_training must be
 * set (GNF_EINVAL otherwise).
 * ws: gnf_timestep_gnn_workspace_bytes, as for gnf_timestep_gnn_f32.
 *
 * ---- backward ----------------------------------------------------------------------------------------------------------
 * gnf_timestep_gnn_backward_f32: given g_out = dL/d out [n_nodes][D] (leading dimension ldg; read, never written) it writes
 * dL/d(parameter) for every trainable variable of the encoder, and dL/dx into g_x (nullable; leading dimension ldgx).
 *   csr      the batch's edges grouped by receiver (the forward's csr)
 *   csr_t    the same edges grouped by sender, exactly as gnf_grevnet_backward_f32 takes it
 *   grad     a GnfTimestepGnn of g's shape (num_timesteps, weight_sharing, layer widths, bns / lns present or not).
 *            nets[q].W[j] / b[j] point at gradient buffers of the parameters' shapes and are OVERWRITTEN; with
 *            weight_sharing the T uses of the shared net are summed, in the order the walk meets them (timestep T-1 first,
 *            timestep 0 last: a fixed order).  bns[i].gamma / beta and lns[i].gamma / beta point at their gradient buffers
 *            (device fp32 [D], written through the const-qualified members); the moving-statistics and batch-moment members
 *            of grad->bns are ignored, and so are grad's scalar members other than the two shape ones.
 *
 * The walk, with G = dL/d(current rows), starting from G = g_out:
 *   residual        dL/dx receives g_out at the end (out = nodes + x)
 *   for i = T-1 .. 0:
 *     GNN module    recompute from the stashed module input v:  h_0 = combine(v, aggregate(v)),  h_j = act(h_{j-1} W_{j-1}
 *                   + b_{j-1}) for j = 1 .. K-1 (the hidden layers; the output layer is not needed)
 *                   dP_K = G;  for j = K-1 .. 0:  dW_j = h_j^T dP_{j+1},  db_j = colsum dP_{j+1},
 *                                                dP_j = (dP_{j+1} W_j^T) * act'(h_j)   (no act' for j = 0: dP_0 = dL/dh_0)
 *                   act'(h) = 1 where h > 0, else 0 (relu) or alpha (leaky_relu)
 *                   G[u, f] = base(u, f) + sum over edges u -> r of dP_0[r, c0 + f] * w(r)          (along csr_t)
 *                       agg combine:    base = epsilon * dP_0[u, f],  c0 = 0
 *                       concat combine: base = dP_0[u, f],            c0 = D   (the direct half; the aggregated half)
 *                       w(r) = 1 / max(indeg(r), 1) for the mean aggregator (the RECEIVER's in-degree, from csr), else 1
 *     snt.LayerNorm with its input a (the batch norm's output, or the timestep's input rows), per row over the D features:
 *                   a^ = (a - mean_f a) / sqrt(var_f a + GNF_LN_EPS);  dgamma_f = sum_rows G a^,  dbeta_f = sum_rows G
 *                   q = G * gamma;  G = (q - mean_f q - a^ * mean_f(q a^)) / sqrt(var_f a + GNF_LN_EPS)
 *     snt.BatchNorm through the batch moments, with u the timestep's input rows, N = n_nodes:
 *                   u^ = (u - mean) * rsqrt(var + bn_eps);   dbeta_c = sum_rows G,   dgamma_c = sum_rows G u^
 *                   G = gamma * rsqrt(var + bn_eps) * (G - dbeta / N - u^ * dgamma / N)
 *                   (not the flow's bijector backward: there is no log-det term.  The clamp of the variance at 0 takes no
 *                   part in the gradient.  At N = 1: u^ = 0, dgamma = 0 and G = 0 exactly.)
 *   dL/dx = G (+ g_out with residual)
 * Every column / row sum is accumulated in fp64 over a fixed number of partial rows and re-reduced in a fixed order; every
 * weight gradient is a fixed split of the rows into slabs summed in slab order.  No float atomics: two calls on the same
 * inputs give the same bits.  x, g_out and the stash are read only.
 *
 * ws: gnf_timestep_gnn_backward_workspace_bytes (a host computation; 0 for arguments no call accepts):
 *   fp64 norm partials [128][D][4]  |  three fp32 [n_nodes][D] gradient buffers  |  [n_nodes][2] row statistics (lns)  |
 *   h_0 [n_nodes][in0]  |  h_1 .. h_{K-1} [n_nodes][widest hidden layer]  |  two dP buffers [n_nodes][max width]  |
 *   weight-gradient slabs (at most 16 row chunks and 64 MiB)
 *
 * Checked before any launch, with gnf_last_error text (both entry points, in addition to what gnf_timestep_gnn_f32 checks):
 *   GNF_EUNSUPPORTED  a net with an attention front-end; n_nodes > 8 388 480 (= 65535 * 128: the GEMM tile's grid over the node
 *                     axis; both entry points, and both size functions return 0 there); bns with D > 4096 (the backward's
 *                     normalising kernel keeps four fp32 constants per column in LDS: 64 KiB at D = 4096, the most a
 *                     workgroup gets without opting in - twice the forward's 32 KiB)
 *   GNF_EINVAL        !g->is_training; null stash; stash / ws not 8-byte aligned; x and out overlapping (forward);
 *                     null csr_t / grad / g_out; a grad whose num_timesteps, weight_sharing, layer widths or bns / lns
 *                     presence differ from g's, or with a null gradient pointer; g_x overlapping g_out (backward)
 *   GNF_ESHAPE        ldg < D, ldgx < D
 *   GNF_EWORKSPACE    ws_bytes or stash_bytes too small
 * n_nodes == 0: GNF_OK; the forward does nothing, the backward zeroes every gradient buffer and touches nothing else.
 * Asynchronous on `stream`, no host synchronisation, no allocation, one stream: capturable. */
size_t gnf_timestep_gnn_stash_bytes(int64_t n_nodes, int32_t D, const GnfTimestepGnn* g);
int gnf_timestep_gnn_train_forward_f32(const GnfCsr* csr, const GnfTimestepGnn* g, const float* x, int64_t ldx, float* out,
                                       int64_t ldo, int32_t D, void* stash, size_t stash_bytes, void* ws, size_t ws_bytes,
                                       gnf_stream_t stream);
size_t gnf_timestep_gnn_backward_workspace_bytes(int64_t n_nodes, int32_t D, const GnfTimestepGnn* g);
int gnf_timestep_gnn_backward_f32(const GnfCsr* csr, const GnfCsr* csr_t, const GnfTimestepGnn* g, const GnfTimestepGnn* grad,
                                  const float* x, int64_t ldx, const float* g_out, int64_t ldg, float* g_x, int64_t ldgx,
                                  int32_t D, const void* stash, size_t stash_bytes, void* ws, size_t ws_bytes,
                                  gnf_stream_t stream);

#endif /* GNF_TIMESTEP_GNN_TRAIN_H */
