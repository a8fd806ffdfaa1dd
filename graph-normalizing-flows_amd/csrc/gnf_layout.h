// Where everything lives in caller-owned memory (host only): the half-step float scratch, the attention region /
// attention-stash slot and the MLP-row stash slot, as plain structs of float offsets + the function that fills each.
// Every writer and every reader of a layout takes its pointers from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gnf.h"

namespace gnf {

// widest hidden layer of a net (1 without hidden layers or without a net): the row pitch of its activation buffers
inline int hidden_max(const GnfMlp* m) {
    int lmax = 1;
    for (int j = 1; m && j < m->num_layers; ++j) lmax = lmax > m->dims[j] ? lmax : m->dims[j];
    return lmax;
}
inline int hidden_max(const GnfMlp* s, const GnfMlp* t) { return hidden_max(s) > hidden_max(t) ? hidden_max(s) : hidden_max(t); }

// net of (half, timestep i) in GnfFlow.s_nets / t_nets (or a gradient flow's)
inline const GnfMlp* flow_net(const GnfFlow* f, const GnfMlp* nets, int half, int i) {
    return f->weight_sharing ? &nets[half] : &nets[half * f->num_timesteps + i];
}
// nets in each of GnfFlow.s_nets / t_nets
inline int flow_net_count(const GnfFlow* f) { return f->weight_sharing ? 2 : 2 * f->num_timesteps; }

// ---- half-step float scratch -------------------------------------------------------------------------------------
// h0 [n, in0] | per net: A [n, lmax] | B [n, lmax] (ping-pong activations of the layered path, two nets side by side for
// the grouped GEMM launches) | s [n, H] | t [n, H] | attention region.  Message-passing nets on the large-batch kernel
// reuse the room behind the layer-0 rows for their split row tiles: kBigSplitMax flags | kBigSplitMax x 16 x 128 floats
// of s rows (gnf_fused_big.hip).
static constexpr int kLayeredActBufs = 4;
static constexpr int kBigSplitMax = 128;
struct HalfScratch {
    size_t h0, bufA[2], bufB[2], s, t;
    size_t attn_region;           // = the floats in front of it (WorkspacePlan.base_floats)
    size_t split_flags, split_s;  // (the flags are ints)
    bool split_fits() const { return split_s + (size_t)kBigSplitMax * 16 * 128 <= attn_region; }
};
inline HalfScratch half_scratch(int64_t n, int in0, int lmax, int32_t H) {
    const size_t N = (size_t)n, act = N * (size_t)lmax;
    HalfScratch L;
    L.h0 = 0;
    for (int q = 0; q < 2; ++q) L.bufA[q] = N * (size_t)in0 + (size_t)(2 * q) * act, L.bufB[q] = L.bufA[q] + act;
    L.s = N * (size_t)in0 + kLayeredActBufs * act;
    L.t = L.s + N * (size_t)H;
    L.attn_region = L.t + N * (size_t)H;
    L.split_flags = (N * (size_t)in0 + 63) / 64 * 64;
    L.split_s = L.split_flags + kBigSplitMax;
    return L;
}

// ---- attention region of the scratch = one half-step's slot of GnfFlow.attn_stash --------------------------------
// [2][n][P] q | k | v, [2][n][in0] h0, [2][n][heads * v] attended values, [2][n][3 * heads] softmax statistics (running
// max at [h], denominator at [heads + h], the third block is scratch of the backward pass).  The graph scope's q | k | v
// row holds per-head values: P = 2 heads kq + heads v (the edge scope's is 2 heads kq + v).
inline bool attn_is_graph(const GnfAttn* at) { return at && at->scope == GNF_ATTN_GRAPH; }
inline int64_t attn_qkv_width(const GnfAttn* at) {
    return 2 * (int64_t)at->num_heads * at->kq_dim + (attn_is_graph(at) ? (int64_t)at->num_heads : 1) * at->v_dim;
}
inline size_t attn_stats_width(int heads) { return 3 * (size_t)heads; }
struct AttnRegion { size_t qkv[2], h0[2], agg[2], stats[2], total; };
inline AttnRegion attn_region(const GnfAttn* at, int64_t n, int32_t in0) {
    AttnRegion R{};
    if (!at) return R;
    const size_t w[4] = {(size_t)attn_qkv_width(at), (size_t)in0, (size_t)at->num_heads * at->v_dim, attn_stats_width(at->num_heads)};
    size_t* const block[4] = {R.qkv, R.h0, R.agg, R.stats};
    for (int k = 0; k < 4; ++k) {
        block[k][0] = R.total, block[k][1] = R.total + (size_t)n * w[k];
        R.total += 2 * (size_t)n * w[k];
    }
    return R;
}

// ---- one half-step's slot of GnfFlow.mlp_stash (ABI v8): the rows the backward walk would otherwise recompute -----
struct MlpStashLayout {
    size_t h0, act, act_each, st, st_each, mask, slot;  // float offsets inside a slot / floats per slot
    int hidden;                                   // K - 1 kept activations per net
    int ld_act;                                   // row pitch of the hidden activations (widest hidden layer)
    int mld, mask_words;                          // act' ballot words: 16-column tiles per mask row, 64-bit words per 16-node tile
    size_t act_of(int q, int j) const { return act + ((size_t)q * hidden + (j - 1)) * act_each; }  // net q, INPUT of layer j = 1 .. K - 1
    size_t st_of(int q) const { return st + (size_t)q * st_each; }                                 // s (q = 0) / t (q = 1)
};
MlpStashLayout mlp_stash_layout(const GnfMlp* net, int64_t n, int32_t H);  // gnf_fused.hip

// ---- workspace of the per-graph entry points, forward and inverse (byte offsets) ---------------------------------
// the plain call's workspace (gnf_workspace_bytes, 256-aligned) | row sums fp64 [2T][n] | bijector terms fp64 [2T].
// sum z^2 of the inverse call's source rows needs no room: the reduction reads z_src, or (in place) a launch in front of
// the walk leaves each graph's value in its graph_out entry.
struct PerGraphLayout {
    size_t base, row_ld, bn_c, total;
    int slots;  // 2T (2 for a flow without timesteps)
};
inline PerGraphLayout per_graph_layout(size_t plain_bytes, int64_t n, int32_t T) {
    PerGraphLayout L;
    L.slots = 2 * (T > 0 ? T : 1);
    L.base = (plain_bytes + 255) / 256 * 256;
    L.row_ld = L.base;
    L.bn_c = L.row_ld + (size_t)L.slots * (size_t)n * sizeof(double);
    L.total = L.bn_c + (size_t)L.slots * sizeof(double);
    return L;
}

}  // namespace gnf
