/* include/gnf_inverse_per_graph.h - per-graph likelihood of generated graphs from the inverse (sampling) pass of
 * libgnf_hip.so: the counterpart of gnf_grevnet_per_graph_f32 for GRevNet.g.  Included by gnf.h (which defines GnfCsr, GnfFlow,
 * gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to be included on its own. */
#ifndef GNF_INVERSE_PER_GRAPH_H
#define GNF_INVERSE_PER_GRAPH_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * GRevNet.g of gnf_grevnet_from_f32(GNF_INVERSE) - same arguments, the same x, bit for bit, in place (z_src NULL or == x) and
 * out of place - plus the flow's own density of every graph it generated.  For graph g of the batch (rows node_offsets[g] ..
 * node_offsets[g + 1]), with s the value each inverse coupling used (after a residual block's x_cond add, after a layer
 * norm), taken from the conditioning half BEFORE its bijector de-normalises it (gnn.py:349-358):
 *   graph_out[2 g + 0] = logdet_g = - sum over its rows, the 2T half-steps and the features of s
 *                                   + n_g * sum_bijectors sum_f (0.5 log(moving_var_f + epsilon) - log gamma_f)
 *   graph_out[2 g + 1] = sum over its rows and all D features of z^2 - the INPUT rows (in place: taken before the walk
 *                        overwrites them)
 *   sums[k]            = sum over g of graph_out[2 g + k], added in graph order
 * all device fp64, written (not accumulated);  log p(x_g) = -0.5 * graph_out[2g+1] - 0.5 * D * ln(2 pi) * n_g - graph_out[2g].
 * The bijectors of g use constants (the moving statistics), so the graphs of a batch are independent even with batch norm: a
 * graph's values in a batch are those of a single-graph call.  Every half-step runs the per-row instance of the kernel the
 * batch size and net widths select anyway; each row's sum_j s is stored (as + sum s: the sign is applied once, in the
 * reduction) by the one workgroup that owns the row, every reduction is fp64 in a fixed order - no atomics, two calls give the
 * same bits.
 * csr->node_offsets / csr->n_graphs >= 1 are REQUIRED for every GNN family; without them, with a null sums / graph_out, or with
 * a bijector that lacks moving statistics: GNF_EINVAL before any launch.  A short workspace: GNF_EWORKSPACE, likewise before
 * any launch.  After any other error (GNF_EHIP: a launch or a runtime call failed part-way) x, graph_out and sums are
 * unspecified - in place, the launch that takes sum z^2 runs in front of the walk.
 * Asynchronous on `stream`, no host synchronisation, capturable like gnf_grevnet_per_graph_f32.  n_nodes == 0: sums and the
 * n_graphs entries are zeroed.  A graph with no nodes gets {0, 0}.  GnfFlow.attn_stash / mlp_stash / bn_allreduce are ignored
 * (nothing in g crosses ranks).
 * ws: gnf_inverse_per_graph_workspace_bytes(n_nodes, n_graphs, D, flow) bytes (a host computation) -
 *   gnf_workspace_bytes (256-aligned) | row sums fp64 [2T][n_nodes] | bijector terms fp64 [2T]
 * (sum z^2 of the source rows needs no room of its own: out of place the reduction reads z_src, in place a launch in front of
 * the walk leaves each graph's value in its graph_out entry). */
size_t gnf_inverse_per_graph_workspace_bytes(int64_t n_nodes, int64_t n_graphs, int32_t D, const GnfFlow* flow);
int gnf_grevnet_inverse_per_graph_f32(const GnfCsr* csr, const GnfFlow* flow, const float* z_src, int64_t ld_src, float* x,
                                      int64_t ld, int32_t D, double* sums /* [2] */,
                                      double* graph_out /* [n_graphs][2]: logdet_g, sum z^2 of graph g */,
                                      void* ws, size_t ws_bytes, gnf_stream_t stream);

/* Which kernels the calling thread's last gnf_grevnet_f32 / _from_f32 / _per_graph_f32 / _inverse_per_graph_f32 call launched
 * for its half-steps: a bit set of GNF_ROUTE_*, 0 before the first call.  Host bookkeeping only (a thread-local word the
 * forward / inverse half-step launchers OR into): how the tests prove that a forced launch shape ran the kernel it names.
 * ONLY those four entry points clear the word on entry: gnf_coupling_half_f32 adds its bits to whatever the word held, and the
 * backward pass (gnf_grevnet_backward_f32) neither clears it nor records its own kernels.  Read it right after one of the four. */
enum GnfRoute {
    GNF_ROUTE_FUSED_16 = 1 << 0,       /* k_half_fused, both nets, 16-row tiles */
    GNF_ROUTE_FUSED_32 = 1 << 1,       /* k_half_fused, both nets, 32-row tiles */
    GNF_ROUTE_FUSED_FRONT = 1 << 2,    /* ... with the attention prologue */
    GNF_ROUTE_FUSED_FIXED = 1 << 3,    /* ... at the fixed head geometry */
    GNF_ROUTE_FUSED_GEO = 1 << 4,      /* k_half_fused_geo */
    GNF_ROUTE_ONE_NET_16 = 1 << 5,     /* k_half_fused, one net per workgroup, 16-row tiles (+ a coupling kernel) */
    GNF_ROUTE_ONE_NET_32 = 1 << 6,     /* ... 32-row tiles */
    GNF_ROUTE_BIG = 1 << 7,            /* k_half_big without split row tiles */
    GNF_ROUTE_BIG_SPLIT = 1 << 8,      /* k_half_big with split row tiles */
    GNF_ROUTE_LAYERED = 1 << 9,        /* the layered path (+ a coupling kernel) */
    GNF_ROUTE_COUPLING = 1 << 10,      /* k_coupling */
    GNF_ROUTE_COUPLING_ROWS = 1 << 11, /* k_coupling_rows */
    GNF_ROUTE_LAYER_NORM = 1 << 12,    /* the layer-norm pass of an attention block in front of k_coupling */
    GNF_ROUTE_ATTN_PAIR = 1 << 13,     /* an attention front-end outside the fused kernel (launch_attn_pair) */
    GNF_ROUTE_ROW_SUMS = 1 << 14       /* a per-row (sum_j s) instance ran */
};
int64_t gnf_last_route(void);

#endif /* GNF_INVERSE_PER_GRAPH_H */
