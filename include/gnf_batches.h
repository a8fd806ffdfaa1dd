/* include/gnf_batches.h - the batch-assembly entry points of libgnf_hip.so.  Included by gnf.h (which defines gnf_stream_t and the
 * GNF_E* codes and opens the extern "C" block); not meant to be included on its own. */
#ifndef GNF_BATCHES_H
#define GNF_BATCHES_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * The input side of a training step on the device: from "which graphs" (gnf_batch_assemble) or "how many nodes each"
 * (gnf_complete_batch) to the index arrays of a GraphsTuple AND both of its CSRs, without a host loop, an index upload or a
 * sort.  They replace the per-batch host assembly of graph_data.py:113-122 (gn.utils_np.data_dicts_to_graphs_tuple) and of
 * train_grevnet_with_data.py:237-271 (transform_example over utils.py:164-183), and the two gnf_build_csr calls behind each.
 *
 * GnfBatchStore: a dataset of G graphs treated as ONE big batch, resident on the device.
 *   node_off[G + 1]  int32, edge_off[G + 1]  int64: exclusive prefix sums of the dataset's n_node / n_edge.
 *   senders, receivers  int32 [n_edges]: the dataset's edge order, DATASET-WIDE node ids (local id + node_off[g]).
 *   rowptr / col and rowptr_t / col_t: what gnf_build_csr makes of that big batch by receiver and (senders and receivers
 *   swapped) by sender - built once per dataset.  There is no second sorter here.
 *   n_graphs = G, n_nodes = node_off[G], n_edges = edge_off[G] (<= INT32_MAX: rowptr is int32).
 *
 * gnf_batch_assemble: the batch of the graphs graph_ids[0 .. n_batch) (device int32; repeats allowed, any order).  Writes
 *   n_node[B], n_edge[B], node_offsets[B + 1]                      the batch's sizes and the exclusive prefix sum of n_node
 *   senders[E], receivers[E]                                       graph by graph in dataset edge order
 *   rowptr[N + 1], col[E], rowptr_t[N + 1], col_t[E]               both CSRs of the batch
 * with every node id rebased as  id - node_off[g] + node_offsets[b]  and every row start as
 * rowptr_all[..] - edge_off[g] + (edges of the batch in front of slot b).
 * Contract: every output equals, integer for integer, what the host route gives - concatenate the graphs' local edge lists
 * with their node offsets added, then gnf_build_csr by receiver and by sender.  Why a cut of the dataset-wide CSR is the
 * batch's CSR: a batch is block-diagonal, so graph g's rows list only g's edges; gnf_build_csr is stable within a receiver
 * (original edge order), and a graph's edge order is the same in the dataset and in the batch; so g's rows are the same list
 * wherever g sits, up to the two offsets.
 * n_nodes = N and n_edges = E are ARGUMENTS: the caller keeps the dataset's n_node / n_edge on the host, sums them over its
 * ids and sizes the outputs - nothing is read back.  Every write is bounded by N, E and B and every read of the store by its
 * n_nodes / n_edges, so a graph id outside [0, G) (clamped into range), or N / E that do not match the ids, give wrong
 * numbers, never an access outside the arrays.
 * Structure: one single-workgroup launch scans the B slots (sizes, offsets, a per-slot table in ws), then ONE fill launch
 * covers all six index arrays: a thread owns four consecutive output words at a 16-byte aligned address (whatever the
 * pointer's own alignment: scalar heads and tails), finds the owning slot by binary search in the batch's offsets (kept in
 * LDS up to GNF_BATCH_LDS_SLOTS slots, read from ws beyond) and stores 16 bytes when the four words lie in one graph.  Work is
 * dealt out over the flat node / edge index, not per graph: a 361-node graph next to a 4-node one costs what its words cost.
 * No atomics, every word has one writer: two calls give the same bits.
 * ws: gnf_batch_assemble_workspace_bytes(n_batch) (a host computation; 0 for n_batch < 0 or > GNF_BATCH_MAX_GRAPHS).
 * GNF_EINVAL: null pointers (store, its arrays, graph_ids, outputs, ws; edge arrays may be NULL when the store or the batch has
 * no edges); GNF_ESHAPE: negative sizes, n_batch > GNF_BATCH_MAX_GRAPHS, n_nodes or n_edges (the batch's or the store's) above
 * INT32_MAX; GNF_EWORKSPACE: short workspace - all before any launch.  n_batch == 0 or n_nodes == 0: GNF_OK, rowptr[0] =
 * rowptr_t[0] = 0 and nothing else is written.  Asynchronous on `stream`, no host synchronisation, no allocation. */
#define GNF_BATCH_MAX_GRAPHS (1 << 20)
#define GNF_BATCH_LDS_SLOTS 4095
typedef struct GnfBatchStore {
    const int32_t* node_off; /* [n_graphs + 1] */
    const int64_t* edge_off; /* [n_graphs + 1] */
    const int32_t *senders, *receivers; /* [n_edges] */
    const int32_t *rowptr, *col;        /* [n_nodes + 1], [n_edges]: by receiver */
    const int32_t *rowptr_t, *col_t;    /* the same by sender */
    int64_t n_graphs, n_nodes, n_edges;
} GnfBatchStore;
size_t gnf_batch_assemble_workspace_bytes(int64_t n_batch);
int gnf_batch_assemble(const GnfBatchStore* store, const int32_t* graph_ids, int64_t n_batch, int64_t n_nodes, int64_t n_edges,
                       int32_t* n_node, int32_t* n_edge, int32_t* node_offsets, int32_t* senders, int32_t* receivers,
                       int32_t* rowptr, int32_t* col, int32_t* rowptr_t, int32_t* col_t, void* ws, size_t ws_bytes,
                       gnf_stream_t stream);

/* gnf_complete_batch: the complete topology with self loops of a batch with n_node[0 .. n_batch) nodes (device int32; a
 * negative entry counts as 0), in the sender-major order of utils.py:164-183: graph b's edge k * n_b + l is
 * (node_offsets[b] + k) -> (node_offsets[b] + l).  Writes
 *   node_offsets[B + 1], n_edge[B] = n_b^2, rowptr[N + 1], senders[E], receivers[E].
 * THE ARRAY IDENTITY: for this topology the receiver-sorted CSR is (rowptr, receivers) and the sender-sorted CSR is
 * (rowptr, receivers) too - by receiver, row l of graph b lists the senders of (k -> l) for k ascending (edge order), that is
 * node_offsets[b] + 0 .. n_b - 1; by sender, row k lists the receivers of (k -> l) for l ascending, the same run; and
 * receivers[] itself is that run once per row.  Both rowptrs are the exclusive prefix sum of n_b repeated n_b times.  So no
 * col array is written: pass `receivers` as col of both orientations.
 * n_nodes = N = sum n_b and n_edges = E = sum n_b^2 are arguments, as above; writes are bounded by them whatever n_node holds.
 * Structure, stores and determinism as gnf_batch_assemble (one scan launch, one fill launch over three arrays).
 * ws: gnf_complete_batch_workspace_bytes(n_batch).  GNF_EINVAL: null pointers; GNF_ESHAPE: negative sizes, n_batch >
 * GNF_BATCH_MAX_GRAPHS, n_nodes or n_edges above INT32_MAX (rowptr is int32: sum n_b^2 has to fit); GNF_EWORKSPACE: short
 * workspace - all before any launch.  n_batch == 0 or n_nodes == 0: GNF_OK, rowptr[0] = 0 and nothing else is written. */
size_t gnf_complete_batch_workspace_bytes(int64_t n_batch);
int gnf_complete_batch(const int32_t* n_node, int64_t n_batch, int64_t n_nodes, int64_t n_edges, int32_t* node_offsets,
                       int32_t* n_edge, int32_t* rowptr, int32_t* senders, int32_t* receivers, void* ws, size_t ws_bytes,
                       gnf_stream_t stream);

#endif /* GNF_BATCHES_H */
