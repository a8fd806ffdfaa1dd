/* include/gnf_triplet_loss.h - the sampled triplet loss entry points of libgnf_hip.so.  Included by gnf.h (which defines GnfCsr,
 * gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to be included on its own. */
#ifndef GNF_TRIPLET_LOSS_H
#define GNF_TRIPLET_LOSS_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * triplet_loss of the reference (loss.py:221-270, with the distance functions of loss.py:13-62, 210-218), the loss behind
 * run_gnn.py --loss_type triplet (run_gnn.py:82-91, 155-170, 249-252), and its gradient with respect to the embeddings - on
 * the device, from the sender-grouped CSR of the true batch, in O(N * L) memory: the dense [N, N] true_adj, inv_true_adj and
 * distances of the reference, their row normalisation and tf.distributions.Categorical are not built.
 *
 * The mathematics.  All node ids are batch-global; i runs over the nodes, l over the L = num_sampling_loops rounds.
 *   positive   j+ ~ Categorical(true_adj[i, :] / sum), true_adj[i, j] = the number of edges with sender i and receiver j
 *              (loss.py:66-70): a duplicate edge weighs double, a self loop is a candidate
 *   negative   j- ~ uniform over the nodes j != i of i's own graph without an edge i -> j (loss.py:255-257)
 *   scores     p = s(i, j+), q = s(i, j-), s(i, i) = 0 whatever the score (loss.py:261 zeroes the diagonal) and otherwise, with
 *              d2 = the fp32 fmaf chain over the features in ascending order of (z_i[f] - z_j[f])^2 (as gnf_pred_adj_f32 forms
 *              it) and dot = the same chain of the products z_i[f] z_j[f]:
 *                GNF_TRIPLET_L2               d2                                               (loss.py:210-214)
 *                GNF_TRIPLET_DOT              dot                                              (loss.py:217-218)
 *                GNF_TRIPLET_EXP_L2           exp(-d2)                                         (loss.py:13-18)
 *                GNF_TRIPLET_SIGMOID_L2       sigmoid(temp * (shift - d2 * scale)), scale = 1 / sqrtf((float)D) or 1
 *                                             (scale_by_sqrt_dim; the logit as gnf_adj_loss_dist_f32 spells it; loss.py:36-62)
 *                GNF_TRIPLET_HACKY_CAUCHY_L2  atan(-(d2 - 4)) / pi + 0.5                       (loss.py:27-33)
 *                GNF_TRIPLET_SIGMOID_DOT      sigmoid(dot - 0.5)                               (loss.py:21-24)
 *   term       GNF_TRIPLET_MARGIN: max(margin - p + q, 0) (loss.py:221-222; 0.65 there);  GNF_TRIPLET_RELATIVE: p / (p + q)
 *              (loss.py:225-226)
 *   output     loss_per_node[i] = the sum of i's L terms (unreduced_loss of run_gnn.py:250)
 *
 * Six departures from the reference.
 * 1. The random stream (TF's cannot be reproduced).  A draw is a 32-bit integer r; of cnt candidates it chooses number
 *    k = ((uint64_t)r * cnt) >> 32 - integer arithmetic, the same on the host and on the device.  r comes from `draws`,
 *    uint32 [L][2][N] on the device ([l][0][i] the positive draw, [l][1][i] the negative one), or without it from a hash of
 *    (seed, l, which, i), which = 0 positive / 1 negative, all in wrapping 64-bit arithmetic:
 *      x = seed ^ (0x9E3779B97F4A7C15 * (i + 1)) ^ (0xBF58476D1CE4E5B9 * (2 l + which + 1));
 *      x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31;  r = x >> 32.
 *    Candidate order: positives are the valid entries of row i of the sender-grouped CSR in edge order (multiplicity weighs as
 *    in the reference); negatives are the unset columns of i's out-row in ascending node order, i itself left out.
 * 2. Edges that leave i's graph are ignored, as gnf_adj_loss_f32 ignores them (the data sets hold none).
 * 3. A node without a candidate of either kind (no out-edge; every other node of its graph is a neighbour; a 1-node graph):
 *    the reference hands 0 / 0 to Categorical, which is undefined.  Here every term of such a node is 0, carries no gradient
 *    and is counted in skipped_terms[g]; so is a GNF_TRIPLET_RELATIVE term whose p + q == 0.
 * 4. self_loops: GNF_TRIPLET_SELF_KEEP is the reference (a self loop is a positive candidate and scores 0);
 *    GNF_TRIPLET_SELF_SKIP makes self loops non-candidates.
 * 5. The reduction.  run_gnn.py:270 adds sum_loss, which its triplet branch never defines (a NameError while the graph is
 *    built); sums2[0] = the sum of loss_per_node over the nodes is what a trainer minimises here.
 * 6. No dense pred_adj (loss.py:268): gnf_pred_adj_f32 provides it; the edge-error figures of run_gnn.py:258-264 come from
 *    gnf_adj_loss_f32 without a gradient, counted inside graphs (the reference's unmasked matrix also counts pairs across
 *    graphs). */
enum {
    GNF_TRIPLET_L2 = 0,
    GNF_TRIPLET_DOT = 1,
    GNF_TRIPLET_EXP_L2 = 2,
    GNF_TRIPLET_SIGMOID_L2 = 3,
    GNF_TRIPLET_HACKY_CAUCHY_L2 = 4,
    GNF_TRIPLET_SIGMOID_DOT = 5
};
enum { GNF_TRIPLET_MARGIN = 0, GNF_TRIPLET_RELATIVE = 1 };
enum { GNF_TRIPLET_SELF_KEEP = 0, GNF_TRIPLET_SELF_SKIP = 1 };
#define GNF_TRIPLET_MAX_LOOPS 64
#define GNF_TRIPLET_MAX_NODES 65536

typedef struct GnfTripletSpec {
    int32_t score;              /* GNF_TRIPLET_L2 ... GNF_TRIPLET_SIGMOID_DOT */
    float temp, shift;          /* GNF_TRIPLET_SIGMOID_L2 only */
    int32_t scale_by_sqrt_dim;  /* GNF_TRIPLET_SIGMOID_L2 only; 0: scale = 1 */
    int32_t loss;               /* GNF_TRIPLET_MARGIN / GNF_TRIPLET_RELATIVE */
    float margin;               /* GNF_TRIPLET_MARGIN only */
    int32_t num_sampling_loops; /* L, 1 .. GNF_TRIPLET_MAX_LOOPS */
    int32_t self_loops;         /* GNF_TRIPLET_SELF_KEEP / GNF_TRIPLET_SELF_SKIP */
    uint64_t seed;              /* read without `draws` */
} GnfTripletSpec;

/* csr_t is the SENDER-grouped CSR of the true batch (gnf_build_csr with senders and receivers exchanged: row i lists the
 * receivers of i's out-edges in edge order); csr_t->node_offsets / csr_t->n_graphs are REQUIRED.
 *   loss_per_node  fp32 [n_nodes]: the row's terms are added in fp64 in a fixed order and rounded once; 0 for a row in no graph
 *   loss_per_graph fp64 [n_graphs]: the rows' fp64 sums, added in a fixed order
 *   sums2          fp64 [2]: { sum_g loss_per_graph[g], that / kept terms }, kept = sum_g n_node[g] L - skipped_terms[g]; the
 *                  second entry is 0 when no term is kept
 *   skipped_terms  int64 [n_graphs] (departure 3)
 *   pos_index, neg_index  NULL, or int32 [L][n_nodes]: j+ and j- of (l, i) as batch-global node ids, -1 where the term is
 *                  skipped
 *   grad           NULL, or fp32 [n_nodes][ld_grad], columns 0..D-1 written (every row: zeros where no graph covers it):
 *                  grad_scale * d sums2[0] / d z.  With c = dterm/dscore * dscore/d(d2 or dot) of a pair (i, j): a d2 score adds
 *                  2 c (z_i - z_j) to row i and 2 c (z_j - z_i) to row j, a dot score c z_j to row i and c z_i to row j.  A pair
 *                  with c == 0 (an inactive hinge, a self-loop positive) adds exactly nothing.  Row j sums its own 2 L pairs
 *                  in loop order (positive, then negative), then the pairs of other nodes that chose j in ascending
 *                  (i, l, which): no floating-point atomics anywhere, two calls on the same input give the same bits.
 * max_nodes_per_graph: any upper bound on n_node, at most GNF_TRIPLET_MAX_NODES; a graph larger than the bound is the
 * caller's error: its surplus rows are dropped.  Offsets that do not describe the batch give wrong numbers, never an access
 * outside the arrays.
 * ws: gnf_triplet_loss_workspace_bytes (a host computation; 0 for arguments out of range), O(n_nodes * L):
 *   chosen node int32 [n_nodes][2 L]  |  coefficient fp32 [n_nodes][2 L]  |  pairs by chosen node int32 [n_nodes][2 L]  |
 *   row loss fp64 [n_nodes]  |  row skipped, incoming count, first, cursor int32 [n_nodes] each      (rounded up to 8 bytes)
 * GNF_EINVAL: null pointers (csr_t, spec, sums2, z, ws, loss_per_node, the per-graph outputs, the CSR arrays), missing
 * node_offsets, an unknown score / loss / self_loops; GNF_ESHAPE: D < 1, ld < D, ld_grad < D (with grad), negative sizes,
 * max_nodes_per_graph < 0 or > 65536 (or 0 with nodes), num_sampling_loops outside 1 .. 64, n_nodes * 2 L > INT32_MAX;
 * GNF_EWORKSPACE: short workspace - all before any launch.  n_nodes == 0 or n_graphs == 0: the outputs are zeroed, GNF_OK.
 * Asynchronous on `stream`, no host synchronisation, capturable (`draws` is read on the device at run time: a replay after
 * the tensor was refilled samples anew; `seed` is a host value, fixed at capture). */
size_t gnf_triplet_loss_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int32_t num_sampling_loops);
int gnf_triplet_loss_f32(const GnfCsr* csr_t, const float* z, int64_t ld, int32_t D, int32_t max_nodes_per_graph,
                         const GnfTripletSpec* spec,
                         const uint32_t* draws,                      /* [L][2][n_nodes] or NULL */
                         float* loss_per_node,                       /* [n_nodes] */
                         double* loss_per_graph,                     /* [n_graphs] */
                         double* sums2,                              /* [2]: sum, sum / kept terms */
                         int64_t* skipped_terms,                     /* [n_graphs] */
                         int32_t* pos_index, int32_t* neg_index,     /* [L][n_nodes] or NULL */
                         float* grad, int64_t ld_grad, float grad_scale, /* [n_nodes][ld_grad] or NULL */
                         void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_TRIPLET_LOSS_H */
