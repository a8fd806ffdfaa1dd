/* include/gnf_perturb.h - edge-deletion noise on a batch, with both CSRs of the noisy batch, for the denoising encoder.
 * Included by gnf.h (which defines GnfCsr, gnf_stream_t and the GNF_E* codes and opens the extern "C" block); not meant to be
 * included on its own. */
#ifndef GNF_PERTURB_H
#define GNF_PERTURB_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * The producer side of run_gnn.py --denoising (run_gnn.py:40-41, 171-186, 238; graph_data.py:206-280): the batch the encoder
 * reads is the true batch with edges deleted at random.  The reference's own perturb_batch deletes nothing
 * (remove_edges_from is commented out at graph_data.py:247 and get_next_train_batch returns the clean batch twice,
 * graph_data.py:279-280); this is therefore a definition, not a port.
 *
 * THE DEFINITION.  A directed edge (s, r), batch-global node ids, belongs to the unordered pair lo = min(s, r),
 * hi = max(s, r).  The pair's draw, in wrapping 64-bit arithmetic:
 *   x = seed ^ (0x9E3779B97F4A7C15 * (lo + 1)) ^ (0xBF58476D1CE4E5B9 * (hi + 1));
 *   x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31;  r32 = x >> 32;
 * The pair is deleted iff r32 < threshold, threshold = (uint64_t)(deletion_prob * 4294967296.0): the product is exact in
 * double (a power of two), so host and device agree; deletion_prob = 1.0 gives 2^32 and deletes every pair, 0.0 deletes none.
 * Consequences:
 *   - both directions of an undirected edge share one fate, and so does every duplicate of an edge: a symmetric graph stays
 *     symmetric;
 *   - the same graph at two slots of a batch gets different noise, because its batch-global ids differ;
 *   - no owning-graph lookup is needed to decide an edge;
 *   - an edge that leaves its graph is decided like any other edge and is never used as an index.
 * Self loops.  GNF_PERTURB_LOOPS_KEEP (the default): a loop (i, i) is never deleted - the data sets carry one loop per node on
 * purpose (graph_data.py:43) and the message-passing nets need it.  GNF_PERTURB_LOOPS_DRAW: the pair (i, i) is drawn like any
 * other, which is what the reference's loop over new_g.edges() would do.
 * The seed is the host value `seed`, or - seed_dev != NULL - the word the kernels read from the device at run time: a captured
 * call replayed after the word was changed draws fresh noise (as `draws` does for gnf_triplet_loss_f32). */
enum { GNF_PERTURB_LOOPS_KEEP = 0, GNF_PERTURB_LOOPS_DRAW = 1 };

typedef struct GnfPerturbSpec {
    double deletion_prob;     /* in [0, 1]; NaN or outside: GNF_EINVAL */
    uint64_t seed;            /* read without seed_dev */
    const uint64_t* seed_dev; /* NULL, or one device word read at run time */
    int32_t self_loops;       /* GNF_PERTURB_LOOPS_KEEP / GNF_PERTURB_LOOPS_DRAW */
} GnfPerturbSpec;

/* gnf_perturb_edges: the noisy batch of a batch given as its edge list AND both of its CSRs (csr by receiver, csr_t by sender;
 * csr->node_offsets / csr->n_graphs and csr_t's are REQUIRED; B = n_graphs, N = n_nodes, E = n_edges are csr's, and csr_t must
 * carry the same three).  One call does all launches.  Every edge array below has room for E (E' <= E): there is no count /
 * fill pair and no capacity argument.
 *   senders_out, receivers_out  [E]   the surviving edges in their original order (stable)
 *   rowptr_out [N + 1], col_out [E], rowptr_t_out [N + 1], col_t_out [E]   each row's surviving entries in their original order
 *   n_edge_out [B]              survivors in each graph's segment of the edge list (the segments n_edge describes)
 *   num_removed [B]             n_edge - n_edge_out, counted in directed entries
 *   totals  int64 [2]           { E', E - E' }
 * Words past E' in the edge arrays are unspecified and must not be relied on.
 * Contract: every output equals, integer for integer, the host route - filter the edge list with the mask above, then
 * gnf_build_csr by receiver and by sender on what is left.  Why compacting each of the three arrays on its own gives that: a
 * deletion is a pure function of the pair, so the edge list and the two CSRs agree on which entries go; gnf_build_csr is stable
 * within a row, so a row's survivors keep the order they had.
 * Structure: pass 1, one launch over the three arrays in 64-entry words - a wave decides 64 consecutive entries (the edge list
 * reads s and r; a CSR array finds the row of entry k by binary search in its rowptr) and writes the 64-bit ballot word of
 * survivors; pass 2, one workgroup: the exclusive prefix sums of the words' popcounts per array and of n_edge; pass 3, one
 * launch: entry k with its bit set goes to base[k >> 6] + popcount(word & below(k & 63)), rowptr_out[i] is that same rank
 * evaluated at rowptr[i], n_edge_out[b] the difference of two such ranks on the edge list.  Work is dealt out over the flat
 * entry index, not per row or per graph: a 361-node complete graph next to a 4-node path costs what its words cost.
 * Every output word has one writer, no atomics on positions, no floating point on the device: two calls give the same bits.
 * Every value of rowptr / n_edge that is used as an index is clamped to [0, E], every loop is bounded by E, N or B: arrays
 * that do not describe the batch give wrong numbers, never an access outside the arrays.
 * ws: gnf_perturb_edges_workspace_bytes(n_graphs, n_nodes, n_edges) (a host computation; 0 for arguments no call accepts):
 *   ballot words uint64 [3][W], W = ceil(E / 64)  |  base int32 [3][W + 1]  |  segment starts int32 [B + 1]   (rounded to 8)
 * GNF_EINVAL: null pointers (spec, csr, csr_t, outputs, ws, n_edge, the CSR arrays; edge arrays may be NULL when E == 0),
 * missing node_offsets, an unknown self_loops, a deletion_prob that is NaN or outside [0, 1]; GNF_ESHAPE: negative sizes,
 * n_nodes / n_edges / n_graphs above INT32_MAX, csr_t's sizes unlike csr's; GNF_EWORKSPACE: short workspace - all before any
 * launch, gnf_last_error() starts with the function's name.  n_graphs == 0 or n_nodes == 0: GNF_OK, rowptr_out[0] =
 * rowptr_t_out[0] = 0, totals zeroed, nothing else written.
 * Asynchronous on `stream`, no host synchronisation, no allocation, capturable (deletion_prob and `seed` are host values,
 * fixed at capture; seed_dev is read at run time). */
size_t gnf_perturb_edges_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int64_t n_edges);
int gnf_perturb_edges(const int32_t* senders, const int32_t* receivers, /* [E] */
                      const int32_t* n_edge,                            /* [B], device */
                      const GnfCsr* csr, const GnfCsr* csr_t, const GnfPerturbSpec* spec,
                      int32_t* senders_out, int32_t* receivers_out,     /* [E] */
                      int32_t* rowptr_out, int32_t* col_out,            /* [N + 1], [E] */
                      int32_t* rowptr_t_out, int32_t* col_t_out,        /* [N + 1], [E] */
                      int32_t* n_edge_out, int32_t* num_removed,        /* [B] */
                      int64_t* totals,                                  /* [2] */
                      void* ws, size_t ws_bytes, gnf_stream_t stream);

#endif /* GNF_PERTURB_H */
