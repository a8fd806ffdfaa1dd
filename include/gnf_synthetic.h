/* include/gnf_synthetic.h - the GRevNet driver's synthetic datasets (two moons, mixtures of Gaussians) generated on the device
 * as ready batches: node features, the complete topology with self loops and both of its CSRs.
 * Included by gnf.h (which defines gnf_stream_t and the GNF_E* codes and opens the extern "C" block) after gnf_batches.h (for
 * GNF_BATCH_MAX_GRAPHS); not meant to be included on its own. */
#ifndef GNF_SYNTHETIC_H
#define GNF_SYNTHETIC_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * Replaces, per training iteration of run_grevnet.py, the host work of grevnet_synthetic_data.py:17-21 (the complete digraph
 * with self loops), 28-47 (one data dict per graph), 50-79 (moons / mixture-of-moons / mixture-of-Gaussians samples) and 82-114
 * (the dataset table), the upload of the concatenated dicts and the two gnf_build_csr calls behind them.  The reference draws
 * from numpy / sklearn RandomStates seeded per graph; those streams cannot be continued on a device, so the RANDOMNESS here is
 * a definition (as gnf_perturb.h's is), while the point sets, the topology and the edge order are the reference's.
 *
 * THE DRAW.  gnf_syn_draw(seed, graph, index, stream) -> 32 bits, in wrapping 64-bit arithmetic (plain C below):
 *   mix64(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31   (gnf_perturb.h's)
 *   x = mix64(seed + 0x9E3779B97F4A7C15 * (graph + 1));
 *   x = mix64(x ^ (0xBF58476D1CE4E5B9 * (index + 1)));
 *   x = mix64(x ^ (0x94D049BB133111EB * (stream + 1)));
 *   draw = x >> 32
 * Streams: GNF_SYN_STREAM_KEY 0 the shuffle key of template index i; GNF_SYN_STREAM_U1 / _U2 1 / 2 the two uniforms of node j;
 * GNF_SYN_STREAM_ANGLE 3 the rotation angle of the graph (index 0); GNF_SYN_STREAM_CHOICE 4 the choice of the graph (index 0).
 * The seed is the host value `seed`, or - seed_dev != NULL - the word the kernels read from the device at run time (as
 * GnfPerturbSpec does it): a captured call replayed after the word was changed draws a fresh batch.  The kernels never write
 * the seed word.
 *
 * CHOICES (host side; the library never sees them).  choice = (draw(seed, b, 0, 4) * n_choices) >> 32.  mom_* pick n_b from
 * n_samples_choices with it; mog_4_6 / mog_4_9 pick the offset set, and n_b is the set's size.  The caller uploads n_node[B]
 * (and set_id[B]).
 *
 * SHUFFLE.  idx = the stable argsort of key_i = draw(seed, b, i, 0), i in [0, n_b): ties are broken by i.  Node j of the graph
 * takes template point (moons) or offset (mog) idx[j]; equivalently template index i lands on node rank(i) = #{i' : key_i' <
 * key_i, or key_i' == key_i and i' < i}.  source[node_offsets[b] + j] = idx[j] tells which moon (idx < n_b / 2: the outer one)
 * or which mixture component a node came from.
 *
 * MOONS TEMPLATE (sklearn.datasets.make_moons' point set).  n_out = n / 2, n_in = n - n_out; outer point i: (cos t, sin t),
 * t = pi * i / (n_out - 1); inner point i': (1 - cos t, 0.5 - sin t), t = pi * i' / (n_in - 1); t = 0 when the count is 1;
 * outer points first.  On the device in fp32: t = (float)i * (PI_F / (float)(m - 1)), PI_F = 3.14159265358979f.
 *
 * GAUSSIAN PAIR OF NODE j (Box-Muller on 24-bit uniforms, both exact in fp32):
 *   u1 = ((draw1 >> 8) + 1) * 2^-24 in (0, 1];  u2 = (draw2 >> 8) * 2^-24 in [0, 1);
 *   r = sqrtf(-2 logf(u1));  z0 = r cosf(2 pi u2);  z1 = r sinf(2 pi u2)           (2 pi as the fp32 constant 6.28318530717959f)
 *
 * FEATURES.  moons: x_j = template[idx[j]] + noise * z_j, noise >= 0; noise == 0 gives the template exactly as computed (the
 * product is not formed).  mog: x_j = z_j + offsets[set][idx[j]]; with `rotate` the graph is turned by angle = (draw3 >> 8) *
 * 2^-24 * pi as at grevnet_synthetic_data.py:73-78: (x cos a - y sin a, x sin a + y cos a).  A node index at or beyond the
 * set's size takes offset (0, 0): wrong counts give wrong numbers, never an access outside the arrays.
 *
 * TOLERANCE against a float64 restatement.  Each of the device's logf, sqrtf, cosf, sinf is taken as within 2 ulp (2.4e-7
 * relative).  u1 >= 2^-24, so -2 ln u1 <= 33.3 and r <= 5.77.  r: 2 ulp of the logarithm is 1 ulp of its root, the product
 * by -2 is exact, sqrtf adds 2: |dr| <= 3.5 ulp * 5.77 = 2.4e-6.  The angle 2 pi u2 <= 6.2832: the fp32 constant is off by
 * 2.8e-8 relative and the product rounds once (6e-8), |d angle| <= 5.5e-7, which moves r cos / r sin by at most 5.77 * 5.5e-7
 * = 3.2e-6 - but dr and the angle term cannot both be at their bound on the same component with |cos| = |sin| = 1, and the
 * function's own 2 ulp adds 1.4e-6 where |cos| is near 1 (where the angle term vanishes): |dz| <= 6e-6.
 *   moons: template error <= 1.5e-6 (the angle <= pi to 4e-7, cosf / sinf 2.4e-7, one subtraction 1.2e-7 on values <= 2) plus
 *     noise * |dz| plus the rounding of the sum (|x| <= 2 + 5.77 noise): atol = 3e-6 + 1e-5 * noise.
 *   mog without rotation: |dz| + one rounding of a sum <= 21: atol = 1e-5.
 *   mog with rotation: values up to 30, angle <= pi known to 4e-7, cosf / sinf 2.4e-7, two products and a sum each 6e-8
 *     relative: 30 * (4e-7 + 2.4e-7 + 1.8e-7) + the unrotated 1e-5 * sqrt(2) = 3.9e-5: atol = 4e-5.
 *
 * TOPOLOGY: the order of fully_connected_edge_list (grevnet_synthetic_data.py:17-21: networkx's adjacency order with the self
 * loop added last).  Graph b has n nodes at node offset o and edge base e0 = sum of n_a^2 over a < b.  Edge e0 + k * n + p is
 * (o + k) -> (o + l) with l = p + (p >= k) for p < n - 1 and l = k for p = n - 1.  n_edge[b] = n^2;
 * rowptr[o + r] = e0 + r * n, rowptr[N] = E.
 * THE ARRAY IDENTITY.  gnf_build_csr is stable in edge order and the edges are sender-major, so by receiver, row r meets the
 * senders 0 .. n - 1 ascending (its own self loop at position r): the CSR is (rowptr, col) with col[e0 + r * n + p] = o + p.
 * By sender, row k lists k's out-edges in edge order: the CSR is (rowptr, receivers).  One rowptr serves both orientations,
 * `receivers` is the by-sender col, and `col` is the only extra array.  (gnf_complete_batch's order has no self-loop-last
 * rule, so there col == receivers as well; here the two differ.) */
enum { GNF_SYN_MOONS = 0, GNF_SYN_MOG = 1 };
enum { GNF_SYN_STREAM_KEY = 0, GNF_SYN_STREAM_U1 = 1, GNF_SYN_STREAM_U2 = 2, GNF_SYN_STREAM_ANGLE = 3, GNF_SYN_STREAM_CHOICE = 4 };
/* the largest graph gnf_synthetic_nodes ranks: a node's rank recomputes the n_b keys of its graph, n_b^2 hashes per graph */
#define GNF_SYN_MAX_NODES 1024
#define GNF_SYN_MAX_SETS 8 /* offset sets of a mixture-of-Gaussians spec */

/* one definition for the host and, under hipcc, for the kernels */
#ifdef __HIPCC__
#define GNF_SYN_FN static inline __host__ __device__
#else
#define GNF_SYN_FN static inline
#endif
GNF_SYN_FN uint64_t gnf_syn_mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
GNF_SYN_FN uint32_t gnf_syn_draw(uint64_t seed, uint64_t graph, uint64_t index, uint64_t stream) {
    uint64_t x = gnf_syn_mix64(seed + 0x9E3779B97F4A7C15ull * (graph + 1ull));
    x = gnf_syn_mix64(x ^ (0xBF58476D1CE4E5B9ull * (index + 1ull)));
    x = gnf_syn_mix64(x ^ (0x94D049BB133111EBull * (stream + 1ull)));
    return (uint32_t)(x >> 32);
}

typedef struct GnfSyntheticSpec {
    uint64_t seed;            /* read without seed_dev */
    const uint64_t* seed_dev; /* NULL, or one device word read at run time */
    int32_t kind;             /* GNF_SYN_MOONS / GNF_SYN_MOG */
    int32_t rotate;           /* mog: 0 / 1 */
    double noise;             /* moons: >= 0 (NaN or negative: GNF_EINVAL); used as (float)noise */
    const float* offsets;     /* mog: device fp32 [n_sets][set_stride][2]; moons: ignored */
    int32_t n_sets;           /* mog: 1 .. GNF_SYN_MAX_SETS */
    int32_t set_stride;       /* mog: points between two sets, >= every set_size */
    int32_t set_size[GNF_SYN_MAX_SETS]; /* mog: points of each set, 0 .. set_stride */
} GnfSyntheticSpec;

/* gnf_synthetic_topology: from n_node[0 .. n_batch) (device int32; a negative entry counts as 0) the arrays of TOPOLOGY above:
 *   node_offsets [B + 1], n_edge [B], rowptr [N + 1], senders [E], receivers [E], col [E].
 * n_nodes = N = sum n_b and n_edges = E = sum n_b^2 are arguments (the caller knows them without reading anything back) and
 * every write is bounded by them whatever n_node holds.
 * Structure and guarantees as gnf_complete_batch: one single-workgroup scan launch (node and edge offsets, n_edge), then ONE
 * fill launch dealt out over the flat word index of the four arrays: a thread owns four consecutive words at a 16-byte aligned
 * address, finds their graph by binary search in the offsets, and stores 16 bytes when the four words lie in one graph and
 * inside the array; heads, tails and groups across a graph boundary store word by word, so any 4-byte pointer alignment is
 * served.  No atomics, every word has one writer, no floating point: two calls give the same bits.
 * ws: gnf_synthetic_topology_workspace_bytes(n_batch) (a host computation, monotone in n_batch; 0 for n_batch < 0 or >
 * GNF_BATCH_MAX_GRAPHS): the edge offsets int32 [B + 1], rounded to 8.
 * GNF_EINVAL: null pointers (edge arrays may be NULL when n_edges == 0); GNF_ESHAPE: negative sizes, n_batch >
 * GNF_BATCH_MAX_GRAPHS, n_nodes or n_edges above INT32_MAX; GNF_EWORKSPACE: short workspace - all before any launch,
 * gnf_last_error() starts with the function's name.  n_batch == 0 or n_nodes == 0: GNF_OK, rowptr[0] = 0, nothing else written.
 * Asynchronous on `stream`, no host synchronisation, no allocation, capturable. */
size_t gnf_synthetic_topology_workspace_bytes(int64_t n_batch);
int gnf_synthetic_topology(const int32_t* n_node, int64_t n_batch, int64_t n_nodes, int64_t n_edges, int32_t* node_offsets,
                           int32_t* n_edge, int32_t* rowptr, int32_t* senders, int32_t* receivers, int32_t* col, void* ws,
                           size_t ws_bytes, gnf_stream_t stream);

/* gnf_synthetic_nodes: the node features of FEATURES above for the batch whose n_node / node_offsets are given (device int32
 * [B] / [B + 1], as gnf_synthetic_topology wrote them); set_id (device int32 [B], NULL = set 0 everywhere; clamped into
 * [0, n_sets)) picks each graph's offset set for mog and is ignored for moons.
 *   nodes   fp32 [N][2] with leading dimension ld >= 2; columns 2 .. ld - 1 are not touched
 *   source  int32 [N] or NULL: idx[j] of SHUFFLE
 * One launch over the flat (graph, template index) space, which is the node index space: thread node_offsets[b] + i computes
 * rank(i) by recomputing the n_b keys of its graph from the hash (no LDS, no barrier, no workspace; a graph may straddle
 * workgroups), computes its point with the Gaussian pair of node rank(i), and writes row node_offsets[b] + rank(i).  Ranks are
 * a permutation of [0, n_b), so every row has one writer; no atomics: two calls give the same bits.
 * max_nodes_per_graph is the caller's bound on n_b, 1 .. GNF_SYN_MAX_NODES (the per-graph cost is n_b^2 hashes: 1024 keeps a
 * 32-graph batch of the largest size near 0.1 ms); a count above it is clamped to it, a negative one is 0.  Every row written
 * is < n_nodes whatever n_node / node_offsets hold.
 * GNF_EINVAL: null pointers (spec, n_node, node_offsets, nodes), unknown kind, noise < 0 or NaN, mog without offsets, with
 * n_sets outside 1 .. GNF_SYN_MAX_SETS, or with a set_size outside 0 .. set_stride; GNF_ESHAPE: negative sizes, n_batch >
 * GNF_BATCH_MAX_GRAPHS, n_nodes above INT32_MAX, ld < 2, max_nodes_per_graph outside 1 .. GNF_SYN_MAX_NODES - all before any
 * launch.  n_batch == 0 or n_nodes == 0: GNF_OK, nothing written.
 * Asynchronous on `stream`, no host synchronisation, no allocation, capturable (the spec's host values are fixed at capture;
 * seed_dev is read at run time). */
int gnf_synthetic_nodes(const GnfSyntheticSpec* spec, const int32_t* n_node, const int32_t* set_id, const int32_t* node_offsets,
                        int64_t n_batch, int64_t n_nodes, int32_t max_nodes_per_graph, float* nodes, int64_t ld, int32_t* source,
                        gnf_stream_t stream);

#endif /* GNF_SYNTHETIC_H */
