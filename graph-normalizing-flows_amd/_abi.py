"""ctypes binding of libgnf_hip.so (the C ABI declared in include/gnf.h).

This is the whole FFI surface: plain pointers and sizes, PyTorch tensors only as the owners of
device memory (`tensor.data_ptr()`) and of the stream (`torch.cuda.current_stream().cuda_stream`).
There is NO fallback: if the HIP library is missing or a call fails, we raise.
"""
import ctypes as C
import os

GNF_MAX_LAYERS = 8
GNF_ABI_VERSION = 10

GNF_AGG_SUM, GNF_AGG_MEAN = 0, 1
GNF_COMBINE_EPS, GNF_COMBINE_CONCAT = 0, 1
GNF_ACT_RELU, GNF_ACT_LEAKY_RELU = 0, 1
GNF_FORWARD, GNF_INVERSE = 0, 1
GNF_ATTN_EDGES, GNF_ATTN_GRAPH = 0, 1   # GnfAttn.scope (ABI v10)
GNF_MMD_GAUSSIAN_EMD, GNF_MMD_GAUSSIAN_TV = 0, 1   # gnf_hist_mmd_f64 kernel
GNF_KEEP_LARGEST_COMPONENT, GNF_KEEP_NON_ISOLATED, GNF_KEEP_MASK = 0, 1, 2   # gnf_graph_subgraph_count rule

_HERE = os.path.dirname(os.path.abspath(__file__))
# GNF_LIB_PATH: developer override (a library built from another checkout, for A/B runs); still a HIP build
LIB_PATH = os.environ.get("GNF_LIB_PATH") or os.path.join(_HERE, "libgnf_hip.so")


class GnfError(RuntimeError):
    pass


class GnfCsr(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("col", C.c_void_p), ("n_nodes", C.c_int64),
                ("n_edges", C.c_int64),
                ("node_offsets", C.c_void_p), ("n_graphs", C.c_int64)]   # ABI v10: graph-scope attention


class GnfAttn(C.Structure):
    _fields_ = [("num_heads", C.c_int32), ("kq_dim", C.c_int32), ("v_dim", C.c_int32), ("out_dim", C.c_int32),
                ("concat", C.c_int32), ("kq_dim_division", C.c_int32), ("residual", C.c_int32),
                ("layer_norm", C.c_int32), ("Wq", C.c_void_p), ("Wk", C.c_void_p), ("Wv", C.c_void_p),
                ("Wo", C.c_void_p), ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p),
                ("scope", C.c_int32)]   # ABI v10: GNF_ATTN_EDGES / GNF_ATTN_GRAPH


class GnfMlp(C.Structure):
    _fields_ = [("num_layers", C.c_int32), ("dims", C.c_int32 * (GNF_MAX_LAYERS + 1)),
                ("W", C.c_void_p * GNF_MAX_LAYERS), ("b", C.c_void_p * GNF_MAX_LAYERS),
                ("packed", C.c_void_p), ("attn", C.POINTER(GnfAttn))]


class GnfGnnSpec(C.Structure):
    _fields_ = [("agg", C.c_int32), ("combine", C.c_int32), ("epsilon", C.c_float),
                ("activation", C.c_int32), ("alpha", C.c_float)]


class GnfBatchNorm(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("moving_mean", C.c_void_p),
                ("moving_variance", C.c_void_p), ("batch_mean", C.c_void_p), ("batch_variance", C.c_void_p),
                ("epsilon", C.c_float), ("reserved", C.c_int32)]


# ABI v5: int hook(void* ctx, double* device_buf, int64_t count, gnf_stream_t stream) - in-place SUM all-reduce
BN_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class GnfFlow(C.Structure):
    _fields_ = [("num_timesteps", C.c_int32), ("weight_sharing", C.c_int32),
                ("s_nets", C.POINTER(GnfMlp)), ("t_nets", C.POINTER(GnfMlp)), ("gnn", GnfGnnSpec),
                ("bns", C.POINTER(GnfBatchNorm)),
                ("bn_allreduce", BN_ALLREDUCE_FN), ("bn_allreduce_ctx", C.c_void_p), ("bn_sync_buf", C.c_void_p),
                ("attn_stash", C.c_void_p), ("attn_stash_bytes", C.c_size_t),
                ("mlp_stash", C.c_void_p), ("mlp_stash_bytes", C.c_size_t)]


class GnfAdjLossSpec(C.Structure):   # include/gnf_adj_loss.h
    _fields_ = [("temp", C.c_float), ("shift", C.c_float), ("scale_by_sqrt_dim", C.c_int32), ("soft_labels", C.c_int32),
                ("label_epsilon", C.c_float), ("abs_tol", C.c_float)]


class GnfTripletSpec(C.Structure):   # include/gnf_triplet_loss.h
    _fields_ = [("score", C.c_int32), ("temp", C.c_float), ("shift", C.c_float), ("scale_by_sqrt_dim", C.c_int32),
                ("loss", C.c_int32), ("margin", C.c_float), ("num_sampling_loops", C.c_int32), ("self_loops", C.c_int32),
                ("seed", C.c_uint64)]


class GnfDistance(C.Structure):      # include/gnf_distance.h
    _fields_ = [("temp", C.c_float), ("shift", C.c_float), ("scale_by_sqrt_dim", C.c_int32), ("params", C.c_void_p)]


class GnfSntBatchNorm(C.Structure):   # include/gnf_timestep_gnn.h: snt.BatchNorm(scale=True) of one encoder timestep
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("moving_mean", C.c_void_p), ("moving_variance", C.c_void_p),
                ("batch_mean", C.c_void_p), ("batch_variance", C.c_void_p)]


class GnfRowNorm(C.Structure):        # include/gnf_timestep_gnn.h: snt.LayerNorm() of one encoder timestep
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p)]


class GnfTimestepGnn(C.Structure):    # include/gnf_timestep_gnn.h
    _fields_ = [("num_timesteps", C.c_int32), ("weight_sharing", C.c_int32), ("nets", C.POINTER(GnfMlp)), ("gnn", GnfGnnSpec),
                ("bns", C.POINTER(GnfSntBatchNorm)), ("lns", C.POINTER(GnfRowNorm)), ("residual", C.c_int32),
                ("is_training", C.c_int32), ("test_local_stats", C.c_int32), ("bn_eps", C.c_float), ("bn_decay", C.c_float)]


_SIGNATURES = {
    "gnf_abi_version": (C.c_int, []),
    "gnf_set_option": (C.c_int, [C.c_char_p, C.c_int64]),
    "gnf_get_option": (C.c_int64, [C.c_char_p]),
    "gnf_attn_stash_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.POINTER(GnfFlow)]),
    "gnf_mlp_stash_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.POINTER(GnfFlow)]),
    "gnf_last_error": (C.c_char_p, []),
    "gnf_packed_floats": (C.c_int64, [C.POINTER(GnfMlp)]),
    "gnf_pack_mlp": (C.c_int, [C.POINTER(GnfMlp), C.c_void_p, C.c_void_p]),
    "gnf_csr_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnf_build_csr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_aggregate_f32": (C.c_int, [C.POINTER(GnfCsr), C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_int64, C.c_void_p]),
    "gnf_gnn_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.POINTER(GnfMlp), C.c_int32]),
    "gnf_gnn_apply_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfMlp), C.POINTER(GnfGnnSpec),
                                    C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.POINTER(GnfFlow)]),
    "gnf_coupling_half_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfMlp), C.POINTER(GnfMlp),
                                        C.POINTER(GnfGnnSpec), C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "gnf_grevnet_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfFlow), C.c_void_p, C.c_int64,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_grevnet_from_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfFlow), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # added within ABI v10: per-graph log-likelihood terms from one batched forward pass
    "gnf_per_graph_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(GnfFlow)]),
    "gnf_grevnet_per_graph_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfFlow), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_pred_adj_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gnf_pred_adj_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # added within ABI v10: sampled embeddings -> edge lists / CSR on the device
    "gnf_adj_edges_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_adj_edges_count_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                          C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]),
    "gnf_adj_edges_fill": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    # added within ABI v10: degree / clustering statistics of a batch of graphs and the MMD of two histogram sets
    "gnf_graph_stats_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_graph_stats": (C.c_int, [C.POINTER(GnfCsr), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_hist_mmd_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnf_hist_mmd_f64": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                   C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.POINTER(GnfFlow)]),
    "gnf_grevnet_backward_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfCsr), C.POINTER(GnfFlow),
                                           C.POINTER(GnfFlow), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_void_p]),
    "gnf_pack_flow": (C.c_int, [C.POINTER(GnfFlow), C.c_void_p]),
    "gnf_bn_post_step_f32": (C.c_int, [C.POINTER(GnfFlow), C.c_int32, C.c_float, C.c_void_p]),
    "gnf_rccl_unique_id": (C.c_int, [C.c_char_p]),
    "gnf_rccl_comm_create": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "gnf_rccl_comm_destroy": (C.c_int, [C.c_void_p]),
    "gnf_rccl_allreduce_sum_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "gnf_adam_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                               C.c_float, C.c_float, C.c_void_p]),
    "gnf_clip_by_value_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p]),
    "gnf_clip_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gnf_clip_by_norm_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_gauss_sumsq_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_graph_orbits.h (included by gnf.h, added within ABI v10): 4-node orbit counts of a batch of graphs and the MMD
# of two sets of mean orbit vectors.  A table of its own, as the header is a file of its own: EXPORTED_SYMBOLS mirrors the
# prototypes written in gnf.h itself, ORBIT_SYMBOLS those of gnf_graph_orbits.h; lib() binds both.
_ORBIT_SIGNATURES = {
    "gnf_graph_orbits_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_graph_orbits": (C.c_int, [C.POINTER(GnfCsr), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "gnf_vec_mmd_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnf_vec_mmd_i64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                  C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_adj_loss.h (included by gnf.h, added within ABI v10): the adjacency reconstruction loss of embeddings against a
# true batch, its edge-error counts and its gradient.  A table of its own for the same reason.
_ADJ_LOSS_SIGNATURES = {
    "gnf_adj_loss_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_adj_loss_f32": (C.c_int, [C.POINTER(GnfCsr), C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(GnfAdjLossSpec),
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_distance.h (included by gnf.h, added within ABI v10): the loss and the two decoders under a distance function given
# as an argument, whose temp / shift may live on the device, and the loss's gradient with respect to them.  A table of its own
# for the same reason.
_DISTANCE_SIGNATURES = {
    "gnf_pred_adj_dist_f32": (C.c_int, [C.POINTER(GnfDistance), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_adj_edges_count_dist_f32": (C.c_int, [C.POINTER(GnfDistance), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                               C.c_int64, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_adj_loss_dist_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_adj_loss_dist_f32": (C.c_int, [C.POINTER(GnfCsr), C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                        C.POINTER(GnfAdjLossSpec), C.POINTER(GnfDistance), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
}

# include/gnf_timestep_gnn.h (included by gnf.h, added within ABI v10): the encoder's forward pass, TimestepGNN with its batch /
# layer norms.  A table of its own for the same reason.
_ENCODER_SIGNATURES = {
    "gnf_timestep_gnn_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.POINTER(GnfTimestepGnn)]),
    "gnf_timestep_gnn_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfTimestepGnn), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_timestep_gnn_train.h (included by gnf.h behind gnf_timestep_gnn.h, added within ABI v10): the encoder's training
# forward that keeps a stash, and its backward pass.  A table of its own for the same reason.
_ENCODER_TRAIN_SIGNATURES = {
    "gnf_timestep_gnn_stash_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.POINTER(GnfTimestepGnn)]),
    "gnf_timestep_gnn_train_forward_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfTimestepGnn), C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_timestep_gnn_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.POINTER(GnfTimestepGnn)]),
    "gnf_timestep_gnn_backward_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfCsr), C.POINTER(GnfTimestepGnn),
                                                C.POINTER(GnfTimestepGnn), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_inverse_per_graph.h (included by gnf.h, added within ABI v10): per-graph likelihood of generated graphs from the
# inverse pass, and the route report the tests read.  A table of its own for the same reason.
_INVERSE_PER_GRAPH_SIGNATURES = {
    "gnf_inverse_per_graph_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(GnfFlow)]),
    "gnf_grevnet_inverse_per_graph_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfFlow), C.c_void_p, C.c_int64, C.c_void_p,
                                                    C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.c_void_p]),
    "gnf_last_route": (C.c_int64, []),
}

# include/gnf_graph_spectra.h (included by gnf.h, added within ABI v10): normalised-Laplacian eigenvalues of a batch of graphs and
# their per-graph histograms.  A table of its own for the same reason.
_SPECTRA_SIGNATURES = {
    "gnf_graph_spectra_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_graph_spectra": (C.c_int, [C.POINTER(GnfCsr), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_graph_components.h (included by gnf.h, added within ABI v10): connected components of a batch of graphs and the
# extraction of node-induced subgraph batches.  A table of its own for the same reason.
_COMPONENT_SIGNATURES = {
    "gnf_graph_components_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_graph_components": (C.c_int, [C.POINTER(GnfCsr), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_graph_subgraph_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_graph_subgraph_count": (C.c_int, [C.POINTER(GnfCsr), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_graph_subgraph_fill": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_graph_hashes.h (included by gnf.h, added within ABI v10): Weisfeiler-Lehman hashes of a batch of graphs and the
# matching of two hash sets (uniqueness / novelty).  A table of its own for the same reason.
_HASH_SIGNATURES = {
    "gnf_graph_hashes_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_graph_hashes": (C.c_int, [C.POINTER(GnfCsr), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_graph_hash_match_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gnf_graph_hash_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_triplet_loss.h (included by gnf.h, added within ABI v10): the sampled triplet loss of embeddings against a true
# batch and its gradient.  A table of its own for the same reason.
GNF_TRIPLET_L2, GNF_TRIPLET_DOT, GNF_TRIPLET_EXP_L2, GNF_TRIPLET_SIGMOID_L2, GNF_TRIPLET_HACKY_CAUCHY_L2, \
    GNF_TRIPLET_SIGMOID_DOT = range(6)
GNF_TRIPLET_MARGIN, GNF_TRIPLET_RELATIVE = 0, 1
GNF_TRIPLET_SELF_KEEP, GNF_TRIPLET_SELF_SKIP = 0, 1
_TRIPLET_SIGNATURES = {
    "gnf_triplet_loss_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_triplet_loss_f32": (C.c_int, [C.POINTER(GnfCsr), C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(GnfTripletSpec),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_batches.h (included by gnf.h, added within ABI v10): a batch and both of its CSRs from graph ids into a device-resident
# dataset, and the complete topology from node counts.  A table of its own for the same reason.
GNF_BATCH_MAX_GRAPHS = 1 << 20


class GnfBatchStore(C.Structure):    # include/gnf_batches.h
    _fields_ = [("node_off", C.c_void_p), ("edge_off", C.c_void_p), ("senders", C.c_void_p), ("receivers", C.c_void_p),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("rowptr_t", C.c_void_p), ("col_t", C.c_void_p),
                ("n_graphs", C.c_int64), ("n_nodes", C.c_int64), ("n_edges", C.c_int64)]


_BATCH_SIGNATURES = {
    "gnf_batch_assemble_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gnf_batch_assemble": (C.c_int, [C.POINTER(GnfBatchStore), C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_complete_batch_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gnf_complete_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/gnf_dw_plan.h (included by gnf.h, added within ABI v10): the backward walk's weight-gradient launch plan as a flat
# int64 record - a debugging and test view with no stability promise.  A table of its own for the same reason.
GNF_DW_ROUTE_STREAMS, GNF_DW_ROUTE_MERGED, GNF_DW_ROUTE_GENERIC = 0, 1, 2
_DW_PLAN_SIGNATURES = {
    "gnf_dw_plan_describe": (C.c_int64, [C.c_int64, C.c_int32, C.POINTER(GnfMlp), C.c_int32, C.c_int64, C.c_size_t, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int64]),
}
# include/gnf_perturb.h (included by gnf.h, added within ABI v10): edge-deletion noise on a batch with both CSRs of the noisy batch.
# A table of its own for the same reason.
GNF_PERTURB_LOOPS_KEEP, GNF_PERTURB_LOOPS_DRAW = 0, 1


class GnfPerturbSpec(C.Structure):   # include/gnf_perturb.h
    _fields_ = [("deletion_prob", C.c_double), ("seed", C.c_uint64), ("seed_dev", C.c_void_p), ("self_loops", C.c_int32)]


_PERTURB_SIGNATURES = {
    "gnf_perturb_edges_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "gnf_perturb_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GnfCsr), C.POINTER(GnfCsr),
                                    C.POINTER(GnfPerturbSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}
# include/gnf_synthetic.h (included by gnf.h, added within ABI v10): the GRevNet driver's synthetic datasets as ready batches.
# A table of its own for the same reason.
GNF_SYN_MOONS, GNF_SYN_MOG = 0, 1
GNF_SYN_MAX_NODES, GNF_SYN_MAX_SETS = 1024, 8


class GnfSyntheticSpec(C.Structure):   # include/gnf_synthetic.h
    _fields_ = [("seed", C.c_uint64), ("seed_dev", C.c_void_p), ("kind", C.c_int32), ("rotate", C.c_int32),
                ("noise", C.c_double), ("offsets", C.c_void_p), ("n_sets", C.c_int32), ("set_stride", C.c_int32),
                ("set_size", C.c_int32 * GNF_SYN_MAX_SETS)]


_SYNTHETIC_SIGNATURES = {
    "gnf_synthetic_topology_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gnf_synthetic_topology": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gnf_synthetic_nodes": (C.c_int, [C.POINTER(GnfSyntheticSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                      C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
}
# include/gnf_random_graphs.h (included by gnf.h, added within ABI v10): G(n, p) / planted partition and Barabasi-Albert graphs as
# edge lists with both CSRs.  A table of its own for the same reason.
GNF_RG_PLANTED, GNF_RG_BARABASI_ALBERT = 0, 1
GNF_RG_BA_DRAWS, GNF_RG_MAX_M, GNF_RG_BA_TABLE_MAX = 256, 64, 32768
GNF_RG_BA_SEED_XOR = 0xA5A5A5A5A5A5A5A5


class GnfRandomGraphSpec(C.Structure):   # include/gnf_random_graphs.h
    _fields_ = [("seed", C.c_uint64), ("seed_dev", C.c_void_p), ("first_graph", C.c_uint64), ("model", C.c_int32),
                ("self_loops", C.c_int32), ("thr_in", C.c_void_p), ("thr_out", C.c_void_p), ("block", C.c_void_p),
                ("n_blocks", C.c_int32), ("max_m", C.c_int32), ("m_dev", C.c_void_p)]


_RANDOM_GRAPH_SIGNATURES = {
    "gnf_random_graph_edges_count": (C.c_int, [C.POINTER(GnfRandomGraphSpec), C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}
# include/gnf_adj_report.h (included by gnf.h, added within ABI v10): the classified edge list of embeddings against a true batch
# with its scores, and exact order statistics of a class's scores.  A table of its own for the same reason.
GNF_SELECT_MAX_Q = 16
_ADJ_REPORT_SIGNATURES = {
    "gnf_adj_report_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "gnf_adj_report_count_f32": (C.c_int, [C.POINTER(GnfCsr), C.POINTER(GnfDistance), C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p]),
    "gnf_adj_report_fill": (C.c_int, [C.POINTER(GnfDistance), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "gnf_score_select_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                       C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
}
# enum GnfRoute: bits of gnf_last_route()
ROUTE_BITS = {name: 1 << k for k, name in enumerate((
    "fused_16", "fused_32", "fused_front", "fused_fixed", "fused_geo", "one_net_16", "one_net_32", "big", "big_split", "layered",
    "coupling", "coupling_rows", "layer_norm", "attn_pair", "row_sums"))}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)
INVERSE_PER_GRAPH_SYMBOLS = tuple(_INVERSE_PER_GRAPH_SIGNATURES)
ORBIT_SYMBOLS = tuple(_ORBIT_SIGNATURES)
ADJ_LOSS_SYMBOLS = tuple(_ADJ_LOSS_SIGNATURES)
ENCODER_SYMBOLS = tuple(_ENCODER_SIGNATURES)
ENCODER_TRAIN_SYMBOLS = tuple(_ENCODER_TRAIN_SIGNATURES)
DISTANCE_SYMBOLS = tuple(_DISTANCE_SIGNATURES)
SPECTRA_SYMBOLS = tuple(_SPECTRA_SIGNATURES)
COMPONENT_SYMBOLS = tuple(_COMPONENT_SIGNATURES)
HASH_SYMBOLS = tuple(_HASH_SIGNATURES)
TRIPLET_SYMBOLS = tuple(_TRIPLET_SIGNATURES)
BATCH_SYMBOLS = tuple(_BATCH_SIGNATURES)
DW_PLAN_SYMBOLS = tuple(_DW_PLAN_SIGNATURES)
PERTURB_SYMBOLS = tuple(_PERTURB_SIGNATURES)
SYNTHETIC_SYMBOLS = tuple(_SYNTHETIC_SIGNATURES)
RANDOM_GRAPH_SYMBOLS = tuple(_RANDOM_GRAPH_SIGNATURES)
ADJ_REPORT_SYMBOLS = tuple(_ADJ_REPORT_SIGNATURES)

_lib = None


def lib():
    """Load libgnf_hip.so once.  Raises GnfError (never falls back) if it is absent or stale."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GnfError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in {**_SIGNATURES, **_ORBIT_SIGNATURES, **_ADJ_LOSS_SIGNATURES, **_ENCODER_SIGNATURES,
                                  **_ENCODER_TRAIN_SIGNATURES, **_DISTANCE_SIGNATURES,
                                  **_INVERSE_PER_GRAPH_SIGNATURES, **_SPECTRA_SIGNATURES,
                                  **_COMPONENT_SIGNATURES, **_HASH_SIGNATURES, **_TRIPLET_SIGNATURES,
                                  **_BATCH_SIGNATURES, **_DW_PLAN_SIGNATURES, **_PERTURB_SIGNATURES,
                                  **_SYNTHETIC_SIGNATURES, **_RANDOM_GRAPH_SIGNATURES, **_ADJ_REPORT_SIGNATURES}.items():
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.gnf_abi_version() != GNF_ABI_VERSION:
            raise GnfError(f"libgnf_hip.so ABI {handle.gnf_abi_version()} != binding {GNF_ABI_VERSION}")
        _lib = handle
        # developer convenience of THIS binding (the library itself never reads the environment):
        # GNF_OPTIONS="dw_grouped=1,force_shape=21" -> gnf_set_option calls, for tools/ and the launch-shape tests
        for item in filter(None, os.environ.get("GNF_OPTIONS", "").split(",")):
            name, _, val = item.partition("=")
            set_option(name.strip(), int(val or 1))
    return _lib


def set_option(name, value):
    """gnf_set_option: process-wide developer option of the library (0 = automatic)."""
    check(lib().gnf_set_option(name.encode(), int(value)), f"gnf_set_option({name})")


def get_option(name):
    return int(lib().gnf_get_option(name.encode()))


def last_route():
    """gnf_last_route as a set of names (ROUTE_BITS): the kernels this thread's last whole-flow call launched."""
    bits = int(lib().gnf_last_route())
    return {name for name, bit in ROUTE_BITS.items() if bits & bit}


def check(rc, what):
    if rc != 0:
        msg = lib().gnf_last_error()
        raise GnfError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def stream_ptr(device=None):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def embeddings(nodes, what):
    """(z, n, d, ld) of an [N, D >= 1] embedding tensor as the pair entry points take it: float32, unit inner stride, row
    stride ld >= D (torch reports any stride, 0 included, for a dimension of 0 or 1 rows)"""
    z = nodes.float()
    if z.dim() != 2 or z.shape[1] < 1:
        raise ValueError(f"{what} takes [N, D] embeddings with D >= 1, got shape {tuple(z.shape)}")
    if z.stride(1) != 1:
        z = z.contiguous()
    n, d = int(z.shape[0]), int(z.shape[1])
    return z, n, d, (int(z.stride(0)) if n > 1 else max(int(z.stride(0)), d))
