// Graph-scope self-attention (GnfAttn.scope == GNF_ATTN_GRAPH): MultiheadSelfAttention / SelfAttention of
// the reference gnn.py:576-738.  Every node attends to every node of its own graph, itself included, whatever the edge
// list says:
//   q = x Wq, k = x Wk [N, heads, kq];  v = x Wv [N, heads, v]   (one value projection per head)
//   logit[h, i, j] = < q[i, h], k[j, h] > (/ sqrt(kq)),  softmax over the j of i's graph;  attended[i, h v + c]
// The reference forms a dense [N, N] logit matrix over the batch and subtracts 1e5 outside the block-diagonal loss_mask
// (loss.py:131-151); the masked terms are exactly 0 in fp32 whenever a row's logits span less than ~1e5, so the softmax is
// taken per graph here (include/gnf.h, GnfAttn.scope).
//
// The core is the edge family's matrix-core flash attention (gnf_attn_core.hip) with the window of a 64-row tile being the
// node range of its rows' graphs (node_offsets, binary search) instead of its CSR rows, a range test per (row, key) instead
// of the multiplicity table, the ATTENDING row's q as the register operand and the window's k rows in LDS, and values per
// head.  O(sum n_g^2) work, O(N) memory, no edge list.  Around it (launch_attn_graph_front): q | k | v = x [Wq | Wk | Wv]
// on the matrix cores in front (k_attn_proj_mfma with the per-head value width; h0[:, :H] = x rides along), and new =
// attended Wo on the generic GEMM tile into h0[:, H:] behind - or, with Wo == NULL (SelfAttention), the core writes the
// attended values straight into h0[:, H:].
#include "gnf_attn_graph_dev.h"
#include "gnf_common.h"

namespace gnf {

struct GraphAttnFwdArgs {
    const float* qkv[2];  // [N, P] q | k | v per net, P = 2 heads kq + heads v
    float* agg[2];        // attended values, row pitch agg_ld (h0 + H when the block has no output projection)
    float* mz[2];         // NULL, or [N, 3 heads]: running max at [h], denominator at [heads + h]
    int64_t agg_ld;
    GraphAttnWin win;
    int32_t nh, kq, v;
    float scale;
};

static constexpr int kGaRows = 64;

// KG: 16-wide k-groups of a head's q / k, VT: 16-column tiles of its v, ST: 16-key tiles per chunk of the window
template <int KG, int VT, int ST>
__global__ __launch_bounds__(256) void k_attn_graph_fwd(const GraphAttnFwdArgs a) {
    constexpr int CH = 16 * ST, VS = CH + 4;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* kt = sm;                  // [16 KG][VS]  k of the chunk's keys (head h), transposed
    float* vt = kt + 16 * KG * VS;   // [16 VT][VS]  their v (head h), transposed
    const int net = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 15, lgrp = lane >> 4;
    const int nh = a.nh, kq = a.kq, vd = a.v, nq = nh * kq, P = 2 * nq + nh * vd, n = a.win.n;
    const int row0 = blockIdx.x * kGaRows;
    const float* __restrict__ qkv = a.qkv[net];
    const int r = row0 + 16 * wave + lrow;
    const bool live = r < n;
    int glo = 0, ghi = 0;  // this lane's row attends to keys [glo, ghi)
    if (live) graph_attn_range(a.win, r, glo, ghi);
    int win_lo, win_hi;
    graph_attn_tile_window(a.win, row0, kGaRows, win_lo, win_hi);
    const int win_n = win_hi - win_lo;
    const int n_chunks = (win_n + CH - 1) / CH;
    const bool vec4 = ((kq | vd | P) & 3) == 0 && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0;

    for (int h = 0; h < nh; ++h) {
        f32x4 qB[KG], O[VT];
#pragma unroll
        for (int g = 0; g < KG; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 16 * g + 4 * lgrp + q;
                qB[g][q] = (live && j < kq) ? qkv[(int64_t)r * P + h * kq + j] : 0.f;
            }
#pragma unroll
        for (int t = 0; t < VT; ++t) O[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        float m_run = -INFINITY, z_run = 0.f;
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int c0 = ch * CH, cn = win_n - c0 < CH ? win_n - c0 : CH;
            __syncthreads();  // (the previous chunk / head has been read)
            core_stage_t<KG, CH>(kt, qkv + nq + h * kq, P, kq, win_lo + c0, cn, tid, vec4);
            core_stage_t<VT, CH>(vt, qkv + 2 * nq + h * vd, P, vd, win_lo + c0, cn, tid, vec4);
            __syncthreads();
            // S^T tiles: lane holds the logits of keys 16 t + 4 lgrp + i for its row lrow
            f32x4 S[ST];
            float cm = -INFINITY;
#pragma unroll
            for (int t = 0; t < ST; ++t) {
                S[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (16 * t < cn) S[t] = core_dot_tile<KG>(kt, VS, t, lrow, lgrp, kq, qB);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int s = 16 * t + 4 * lgrp + i, key = win_lo + c0 + s;
                    const bool in = s < cn && key >= glo && key < ghi;
                    S[t][i] = in ? S[t][i] * a.scale : -INFINITY;
                    cm = fmaxf(cm, S[t][i]);
                }
            }
            cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
            cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
            const float m_new = fmaxf(m_run, cm);
            const float m_safe = m_new == -INFINITY ? 0.f : m_new;  // (no key of the row's graph so far: every weight is 0)
            const float sc = __expf(m_run - m_safe);
            float zs = 0.f;
#pragma unroll
            for (int t = 0; t < ST; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = S[t][i] == -INFINITY ? 0.f : __expf(S[t][i] - m_safe);
                    S[t][i] = p;
                    zs += p;
                }
            zs += __shfl_xor(zs, 16, 64);
            zs += __shfl_xor(zs, 32, 64);
            z_run = z_run * sc + zs;
            m_run = m_new;
#pragma unroll
            for (int t = 0; t < VT; ++t)
                if (16 * t < vd) O[t] *= sc;
#pragma unroll
            for (int t = 0; t < ST; ++t)
                if (16 * t < cn) core_acc_tile<VT>(vt, VS, t, lrow, lgrp, vd, S[t], O);   // O^T += V^T P^T
        }
        // lane holds O^T[v column 16 g + 4 lgrp + i][row lrow]
        if (live) {
            const float inv = z_run > 0.f ? 1.f / z_run : 0.f;
            float* __restrict__ out = a.agg[net] + (int64_t)r * a.agg_ld + h * vd;
#pragma unroll
            for (int g = 0; g < VT; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = 16 * g + 4 * lgrp + i;
                    if (j < vd) out[j] = O[g][i] * inv;
                }
            if (a.mz[net] && lgrp == 0) {
                float* mz = a.mz[net] + (int64_t)r * 3 * nh;
                mz[h] = m_run;
                mz[nh + h] = z_run > 0.f ? z_run : 1.f;
            }
        }
    }
}

template <int KG, int VT, int ST>
static size_t graph_fwd_lds_bytes() {
    return (size_t)16 * (KG + VT) * (16 * ST + 4) * sizeof(float);
}

int launch_attn_graph_front(const GnfAttn* const* at, int nets, int64_t n, const float* x, int64_t ldx, int32_t H, int32_t in0,
                            const int32_t* node_offsets, int64_t n_graphs, float* scratch, float* const* h0_out, hipStream_t st,
                            float* const* agg_out, float* const* mz_out) {
    if (n == 0) return GNF_OK;
    const GnfAttn* a0 = at[0];
    for (int q = 1; q < nets; ++q)
        if (at[q]->num_heads != a0->num_heads || at[q]->kq_dim != a0->kq_dim || at[q]->v_dim != a0->v_dim ||
            at[q]->out_dim != a0->out_dim || at[q]->kq_dim_division != a0->kq_dim_division ||
            (at[q]->Wo == nullptr) != (a0->Wo == nullptr)) {
            set_error("attention blocks of one coupling must have identical hyper-parameters");
            return GNF_ESHAPE;
        }
    if (!node_offsets || n_graphs < 1 || n_graphs > INT32_MAX - 1) {
        set_error("graph-scope attention needs node_offsets of n_graphs >= 1 graphs");
        return GNF_EINVAL;
    }
    const int nh = a0->num_heads, kq = a0->kq_dim, vd = a0->v_dim, NV = nh * vd;
    const AttnRegion R = attn_region(a0, n, in0);
    float* qkv[2] = {scratch + R.qkv[0], scratch + R.qkv[nets > 1 ? 1 : 0]};
    float* h0[2] = {h0_out[0], h0_out[nets > 1 ? 1 : 0]};
    // q | k | v (per-head values: Wv is [H, heads v]) and h0[:, :H) = x
    int rc = launch_attn_proj_mfma(at, nets, n, x, ldx, H, qkv, st, h0, in0, NV);
    if (rc) return rc;
    GraphAttnFwdArgs a;
    const bool project = a0->Wo != nullptr;
    for (int q = 0; q < 2; ++q) {
        const int s = q < nets ? q : 0;
        a.qkv[q] = qkv[s];
        a.agg[q] = !project ? h0[s] + H : (agg_out ? agg_out[s] : scratch + R.agg[s]);
        a.mz[q] = mz_out ? mz_out[s] : nullptr;
    }
    a.agg_ld = project ? NV : in0;
    a.win = GraphAttnWin{node_offsets, (int32_t)n_graphs, (int32_t)n};
    a.nh = nh, a.kq = kq, a.v = vd;
    a.scale = a0->kq_dim_division ? 1.f / sqrtf((float)kq) : 1.f;
    const dim3 grid((unsigned)((n + kGaRows - 1) / kGaRows), (unsigned)nets);
    if (kq <= 16 && vd <= 16) {   // (run_grevnet's default heads: 8 x 10 / 10)
        const size_t lds = graph_fwd_lds_bytes<1, 1, 8>();
        hipLaunchKernelGGL((k_attn_graph_fwd<1, 1, 8>), grid, dim3(256), lds, st, a);
    } else if (kq <= 64 && vd <= 64) {   // (the data driver's: one head of 64 / 64)
        GNF_ONCE_PER_DEVICE(GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_graph_fwd<4, 4, 8>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)));
        const size_t lds = graph_fwd_lds_bytes<4, 4, 8>();
        hipLaunchKernelGGL((k_attn_graph_fwd<4, 4, 8>), grid, dim3(256), lds, st, a);
    } else {
        GNF_ONCE_PER_DEVICE(GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_graph_fwd<16, 16, 4>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)));
        const size_t lds = graph_fwd_lds_bytes<16, 16, 4>();
        hipLaunchKernelGGL((k_attn_graph_fwd<16, 16, 4>), grid, dim3(256), lds, st, a);
    }
    GNF_LAUNCH_CHECK("k_attn_graph_fwd");
    if (!project) return GNF_OK;
    const float* as_[2] = {a.agg[0], a.agg[1]};
    const float* wo[2] = {at[0]->Wo, at[nets > 1 ? 1 : 0]->Wo};
    const float* nob[2] = {nullptr, nullptr};
    float* ys[2] = {h0[0] + H, h0[1] + H};
    return launch_linear_splitk(as_, (int64_t)NV, wo, nob, ys, (int64_t)in0, nets, n, NV, a0->out_dim, GNF_ACT_RELU, 0.f, 0,
                                nullptr, 0, st);
}

}  // namespace gnf
