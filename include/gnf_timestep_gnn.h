/* include/gnf_timestep_gnn.h - the encoder's forward pass: TimestepGNN (gnn.py:183-235) with its norms.  Included by gnf.h
 * (which defines GnfCsr, GnfMlp, GnfGnnSpec, gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to
 * be included on its own. */
#ifndef GNF_TIMESTEP_GNN_H
#define GNF_TIMESTEP_GNN_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * The encoder of the graph auto-encoder (built at run_gnn.py:230-239): num_timesteps GNN module calls in a row on the
 * nodes of one batch, each optionally preceded by a batch norm and / or a layer norm, and a final residual.  This header is
 * the forward pass, in training and in evaluation mode; the training forward that keeps a stash and the backward pass are
 * in gnf_timestep_gnn_train.h.
 *
 *   nodes = x
 *   for i in 0 .. T-1, in this order (gnn.py:219-232):
 *       nodes = BN_i(nodes)   if bns   (gnn.py:220-225)
 *       nodes = LN_i(nodes)   if lns   (gnn.py:226-228)
 *       nodes = GNN_i(nodes)            (gnn.py:229-232; GNN_0 for every i with weight_sharing)
 *   out = nodes + x if residual (gnn.py:233-234, one fp32 add per element), else nodes
 * x is never written (the reference's graph is functional and the residual needs the original rows); x and out must not
 * overlap (GNF_EINVAL).  GNN_i is exactly gnf_gnn_apply_f32 of nets[i] - the same launches, the same bits.
 *
 * BN_i: snt.BatchNorm(scale=True) over the node axis (gnn.py:210-213), a plain normaliser - NOT the flow's bijector
 * (GnfBatchNorm): no log-det term, the moving statistics are used in evaluation and updated in training.
 *   statistics   the batch's moments when is_training || test_local_stats, else moving_mean / moving_variance.
 *                Moments: mean and BIASED variance over the n_nodes rows (tf.nn.moments), accumulated in fp64 from
 *                fixed-order partial sums (two calls on the same input give the same bits), the variance clamped at 0.
 *   arithmetic   tf.nn.batch_normalization: inv = rsqrt(var + bn_eps) * gamma;  y = x * inv + (beta - mean * inv)   (fp32)
 *   update       when is_training, inside the call and on `stream`: moving -= (moving - batch) * (1 - bn_decay) in fp32 for
 *                both statistics - what the UPDATE_OPS dependency of the training step does (run_gnn.py:295-296).  Never
 *                otherwise.  One update per call (per replay of a captured call).
 *   batch_mean / batch_variance (nullable) receive the batch's moments whenever they were taken.
 * UNPINNED upstream facts (Sonnet 1.x is third party and absent; restated from its batch_norm.py): eps = 1e-3 and
 * decay_rate = 0.999 are the constructor defaults the reference leaves untouched; gamma starts at ones, beta at zeros,
 * moving_mean at zeros, moving_variance at ones; the moving variance is updated with the BIASED batch variance (the same
 * tensor that normalises); the update is assign_moving_average without zero-debias, its rate (1 - decay_rate) rounded to fp32.
 * LN_i: snt.LayerNorm() (gnn.py:214-215) as GnfAttn.layer_norm restates it: per row, biased variance over the D features,
 *   (h - mean) / sqrt(var + GNF_LN_EPS) * gamma + beta.
 *
 * All GnfSntBatchNorm / GnfRowNorm pointers are device fp32 [D].  */
typedef struct GnfSntBatchNorm {
    const float* gamma;
    const float* beta;
    float* moving_mean;     /* read when !is_training && !test_local_stats; read and written when is_training */
    float* moving_variance; /* (may be NULL in the one mode that does neither: !is_training && test_local_stats) */
    float* batch_mean;      /* optional outputs, may be NULL */
    float* batch_variance;
} GnfSntBatchNorm;

typedef struct GnfRowNorm {
    const float* gamma;
    const float* beta;
} GnfRowNorm;

typedef struct GnfTimestepGnn {
    int32_t num_timesteps; /* T >= 1 */
    int32_t weight_sharing;
    const GnfMlp* nets;         /* HOST: T descriptors, or 1 with weight_sharing (gnn.py:206-209); attn as in GnfMlp.  Every net
                                   maps the module's input width for D (D; 2 D for GNF_COMBINE_CONCAT; dims[0] with an
                                   attention front-end) to exactly D, and all nets have the same layer widths and front-end
                                   geometry (one make_gnn_fn builds them) */
    GnfGnnSpec gnn;
    const GnfSntBatchNorm* bns; /* HOST: NULL (use_batch_norm=False) or T entries - one per timestep even with weight sharing */
    const GnfRowNorm* lns;      /* HOST: NULL (use_layer_norm=False) or T entries */
    int32_t residual;
    int32_t is_training;
    int32_t test_local_stats;
    float bn_eps;   /* > 0; Sonnet default 1e-3 */
    float bn_decay; /* in [0, 1]; Sonnet default 0.999; read when is_training */
} GnfTimestepGnn;

/* ws: gnf_timestep_gnn_workspace_bytes (a host computation; 0 for arguments no call accepts):
 *   fp64 moment partials [16][D][2] (with bns)  |  two ping-pong buffers fp32 [n_nodes][D]  |  the scratch of one module call
 *   (gnf_gnn_workspace_bytes of nets[0])
 * Checked before any launch, with gnf_last_error text:
 *   GNF_EINVAL      null csr / g / nets / CSR arrays / x / out / ws; bad GnfGnnSpec enums; a bns entry with a null gamma / beta
 *                   or, in a mode that reads or writes them, null moving statistics; bn_eps <= 0; bn_decay outside [0, 1]
 *                   when is_training; an lns entry with a null gamma / beta; graph-scope attention without
 *                   csr->node_offsets; x and out overlapping; ws not 8-byte aligned
 *   GNF_ESHAPE      T < 1, D < 1, ldx < D, ldo < D, a net that does not map the module's input width to D, nets with
 *                   different signatures, an attention geometry outside GnfAttn's limit
 *   GNF_EUNSUPPORTED  bns with D > 4096 (the normalising kernel keeps inv / shift of every column in LDS)
 *   GNF_EWORKSPACE  ws_bytes too small
 * n_nodes == 0: GNF_OK, no device work (the moving statistics stay as they are).  Asynchronous on `stream`, no host
 * synchronisation, no allocation, one stream: capturable like gnf_grevnet_f32. */
size_t gnf_timestep_gnn_workspace_bytes(int64_t n_nodes, int32_t D, const GnfTimestepGnn* g);
int gnf_timestep_gnn_f32(const GnfCsr* csr, const GnfTimestepGnn* g, const float* x, int64_t ldx, float* out, int64_t ldo,
                         int32_t D, void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_TIMESTEP_GNN_H */
