// Backward of the graph-scope attention (forward: gnf_attn_graph.hip; reference gnn.py:576-738 under tf.gradients).  With
// the statistics the forward pass leaves per (row, head) - running max m, denominator Z - and its attended values O:
//   P[i, j]  = exp(scale <q_i, k_j> - m_i) / Z_i  for j in i's graph        the softmax weights, rebuilt on the matrix cores
//   dP[i, j] = < dO_i, v_j >,  delta_i = < dO_i, O_i >,  dS = P (dP - delta_i)
//   dq_i = scale sum_j dS k_j                               row side (k_attn_graph_bwd_rows: a tile of 64 rows, chunks of
//                                                            its graphs' nodes as keys; writes delta for the key side)
//   dk_j = scale sum_i dS q_i,  dv_j = sum_i P dO_i          key side (k_attn_graph_bwd_keys: a tile of 64 keys; the rows
//                                                            that attend to key j are j's own graph: no transposed topology)
// Both are the edge family's matrix-core backward (gnf_attn_core_bwd.hip) with the range test of the forward in place of the
// multiplicity table and values per head.  Then dL/dx_cond += dq Wq^T + dk Wk^T + dv Wv^T + dh0[:, :H] of both nets
// (k_attn_graph_bwd_dx), which also copies the conditioning half for the weight-gradient GEMMs.
#include "gnf_attn_graph_dev.h"
#include "gnf_common.h"

namespace gnf {

struct GraphAttnBwdArgs {
    const float* qkv[2];   // [N, P] q | k | v, P = 2 heads kq + heads v
    const float* dagg[2];  // dL/d(attended values), row pitch dagg_ld
    const float* agg[2];   // attended values of the forward pass, row pitch agg_ld
    float* stats[2];       // [N, 3 heads]  m | Z | delta (delta: written by the row pass, read by the key pass)
    float* dqkv[2];        // [N, P]        dq | dk | dv
    int64_t dagg_ld, agg_ld;
    GraphAttnWin win;
    int32_t nh, kq, v;
    float scale;
};

static constexpr int kGbRows = 64;

// ---- row side: dq ---------------------------------------------------------------------------------------------------------
template <int KG, int VT, int ST>
__global__ __launch_bounds__(256) void k_attn_graph_bwd_rows(const GraphAttnBwdArgs a) {
    constexpr int CH = 16 * ST, VS = CH + 4;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* kt = sm;                  // [16 KG][VS]  k of the chunk's keys, transposed
    float* vt = kt + 16 * KG * VS;   // [16 VT][VS]  their v of head h, transposed
    const int net = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 15, lgrp = lane >> 4;
    const int nh = a.nh, kq = a.kq, vd = a.v, nq = nh * kq, P = 2 * nq + nh * vd, n = a.win.n;
    const int row0 = blockIdx.x * kGbRows;
    const float* __restrict__ qkv = a.qkv[net];
    const int r = row0 + 16 * wave + lrow;
    const bool live = r < n;
    int glo = 0, ghi = 0;
    if (live) graph_attn_range(a.win, r, glo, ghi);
    int win_lo, win_hi;
    graph_attn_tile_window(a.win, row0, kGbRows, win_lo, win_hi);
    const int win_n = win_hi - win_lo, n_chunks = (win_n + CH - 1) / CH;
    const bool vec4 = ((kq | vd | P) & 3) == 0 && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0;
    for (int h = 0; h < nh; ++h) {
        f32x4 qB[KG], dB[VT], dQ[KG];
        float dpart = 0.f;
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            dQ[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 16 * g + 4 * lgrp + q;
                qB[g][q] = (live && j < kq) ? qkv[(int64_t)r * P + h * kq + j] : 0.f;
            }
        }
#pragma unroll
        for (int g = 0; g < VT; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 16 * g + 4 * lgrp + q;
                const bool ok = live && j < vd;
                dB[g][q] = ok ? a.dagg[net][(int64_t)r * a.dagg_ld + h * vd + j] : 0.f;
                dpart += ok ? dB[g][q] * a.agg[net][(int64_t)r * a.agg_ld + h * vd + j] : 0.f;
            }
        dpart += __shfl_xor(dpart, 16, 64);
        dpart += __shfl_xor(dpart, 32, 64);
        const float delta = dpart;
        float* st = a.stats[net] + (int64_t)(live ? r : 0) * 3 * nh;
        const float m = live ? st[h] : 0.f, rz = live ? 1.f / st[nh + h] : 0.f;
        if (live && lgrp == 0) st[2 * nh + h] = delta;   // for the key pass
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int c0 = ch * CH, cn = win_n - c0 < CH ? win_n - c0 : CH;
            __syncthreads();
            core_stage_t<KG, CH>(kt, qkv + nq + h * kq, P, kq, win_lo + c0, cn, tid, vec4);
            core_stage_t<VT, CH>(vt, qkv + 2 * nq + h * vd, P, vd, win_lo + c0, cn, tid, vec4);
            __syncthreads();
#pragma unroll
            for (int t = 0; t < ST; ++t) {
                if (16 * t < cn) {
                    const f32x4 S = core_dot_tile<KG>(kt, VS, t, lrow, lgrp, kq, qB);   // S^T[key 16 t + 4 lgrp + i][row lrow]
                    const f32x4 dW = core_dot_tile<VT>(vt, VS, t, lrow, lgrp, vd, dB);
                    f32x4 dS;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int s = 16 * t + 4 * lgrp + i, key = win_lo + c0 + s;
                        const float p = (s < cn && key >= glo && key < ghi) ? __expf(S[i] * a.scale - m) * rz : 0.f;
                        dS[i] = p * (dW[i] - delta);
                    }
                    core_acc_tile<KG>(kt, VS, t, lrow, lgrp, kq, dS, dQ);
                }
            }
        }
        if (live) {
            float* __restrict__ out = a.dqkv[net] + (int64_t)r * P + h * kq;
#pragma unroll
            for (int g = 0; g < KG; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = 16 * g + 4 * lgrp + i;
                    if (j < kq) out[j] = dQ[g][i] * a.scale;
                }
        }
    }
}

// ---- key side: dk, dv -------------------------------------------------------------------------------------------------------
template <int KG, int VT, int ST>
__global__ __launch_bounds__(256) void k_attn_graph_bwd_keys(const GraphAttnBwdArgs a) {
    constexpr int CH = 16 * ST, VS = CH + 4;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* qt = sm;                   // [16 KG][VS]  q of the chunk's rows (head h), transposed
    float* dt = qt + 16 * KG * VS;    // [16 VT][VS]  their dO of head h, transposed
    float* stl = dt + 16 * VT * VS;   // [3][CH]      m | 1 / Z | delta of head h
    const int net = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 15, lgrp = lane >> 4;
    const int nh = a.nh, kq = a.kq, vd = a.v, nq = nh * kq, P = 2 * nq + nh * vd, n = a.win.n;
    const int row0 = blockIdx.x * kGbRows;
    const float* __restrict__ qkv = a.qkv[net];
    const float* __restrict__ dagg = a.dagg[net];
    const int u = row0 + 16 * wave + lrow;   // this lane's key
    const bool live = u < n;
    int glo = 0, ghi = 0;   // the rows that attend to key u: u's graph
    if (live) graph_attn_range(a.win, u, glo, ghi);
    int win_lo, win_hi;
    graph_attn_tile_window(a.win, row0, kGbRows, win_lo, win_hi);
    const int win_n = win_hi - win_lo, n_chunks = (win_n + CH - 1) / CH;
    const bool vec4q = ((kq | P) & 3) == 0 && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0;
    const bool vec4d = ((vd | a.dagg_ld) & 3) == 0 && (reinterpret_cast<uintptr_t>(dagg) & 15) == 0;
    for (int h = 0; h < nh; ++h) {
        f32x4 kB[KG], vB[VT], dK[KG], dV[VT];
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            dK[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 16 * g + 4 * lgrp + q;
                kB[g][q] = (live && j < kq) ? qkv[(int64_t)u * P + nq + h * kq + j] : 0.f;
            }
        }
#pragma unroll
        for (int g = 0; g < VT; ++g) {
            dV[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 16 * g + 4 * lgrp + q;
                vB[g][q] = (live && j < vd) ? qkv[(int64_t)u * P + 2 * nq + h * vd + j] : 0.f;
            }
        }
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int c0 = ch * CH, cn = win_n - c0 < CH ? win_n - c0 : CH;
            __syncthreads();
            core_stage_t<KG, CH>(qt, qkv + h * kq, P, kq, win_lo + c0, cn, tid, vec4q);
            core_stage_t<VT, CH>(dt, dagg + h * vd, a.dagg_ld, vd, win_lo + c0, cn, tid, vec4d);
            if (tid < CH) {
                const bool ok = tid < cn;
                const float* st = a.stats[net] + (int64_t)(win_lo + c0 + (ok ? tid : 0)) * 3 * nh;
                stl[tid] = ok ? st[h] : 0.f;
                stl[CH + tid] = ok ? 1.f / st[nh + h] : 0.f;
                stl[2 * CH + tid] = ok ? st[2 * nh + h] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < ST; ++t) {
                if (16 * t < cn) {
                    const f32x4 S = core_dot_tile<KG>(qt, VS, t, lrow, lgrp, kq, kB);   // S[row 16 t + 4 lgrp + i][key lrow]
                    const f32x4 dW = core_dot_tile<VT>(dt, VS, t, lrow, lgrp, vd, vB);
                    const f32x4 m4 = *reinterpret_cast<const f32x4*>(stl + 16 * t + 4 * lgrp);
                    const f32x4 z4 = *reinterpret_cast<const f32x4*>(stl + CH + 16 * t + 4 * lgrp);
                    const f32x4 d4 = *reinterpret_cast<const f32x4*>(stl + 2 * CH + 16 * t + 4 * lgrp);
                    f32x4 pw, dS;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int s = 16 * t + 4 * lgrp + i, row = win_lo + c0 + s;
                        pw[i] = (s < cn && row >= glo && row < ghi) ? __expf(S[i] * a.scale - m4[i]) * z4[i] : 0.f;
                        dS[i] = pw[i] * (dW[i] - d4[i]);
                    }
                    core_acc_tile<KG>(qt, VS, t, lrow, lgrp, kq, dS, dK);
                    core_acc_tile<VT>(dt, VS, t, lrow, lgrp, vd, pw, dV);
                }
            }
        }
        if (live) {
            float* __restrict__ ok_ = a.dqkv[net] + (int64_t)u * P + nq + h * kq;
            float* __restrict__ ov = a.dqkv[net] + (int64_t)u * P + 2 * nq + h * vd;
#pragma unroll
            for (int g = 0; g < KG; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = 16 * g + 4 * lgrp + i;
                    if (j < kq) ok_[j] = dK[g][i] * a.scale;
                }
#pragma unroll
            for (int g = 0; g < VT; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = 16 * g + 4 * lgrp + i;
                    if (j < vd) ov[j] = dV[g][i];
                }
        }
    }
}

// ---- dL/dx_cond += dqkv [Wq | Wk | Wv]^T + dh0[:, :H] of both nets -----------------------------------------------------------
// A workgroup owns kGdRows rows; their dqkv rows of one net at a time sit in LDS, a thread owns feature columns and streams
// its row of each weight matrix once per net (kGdRows products per weight load).  No bound on H.
struct GraphAttnDxArgs {
    const float* dqkv[2];
    const float* Wq[2];
    const float* Wk[2];
    const float* Wv[2];
    const float* dh0[2];   // [N, in0]: the concat half [:, :H) goes straight into the gradient
    float* g;
    int64_t ldg;
    const float* xc_src;   // NULL, or copy x_cond [n, H] (row pitch xc_ld) into xc_dst [n][H]
    int64_t xc_ld;
    float* xc_dst;
    int32_t n, H, nq, NV, in0;
};
static constexpr int kGdRows = 16;

__global__ __launch_bounds__(256) void k_attn_graph_bwd_dx(const GraphAttnDxArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // [kGdRows][P]
    const int P = 2 * a.nq + a.NV, H = a.H, tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kGdRows;
    const int rows = (int)(a.n - row0 < kGdRows ? a.n - row0 : kGdRows);
    if (a.xc_dst)
        for (int i = tid; i < rows * H; i += 256) {
            const int rl = i / H, f = i - rl * H;
            a.xc_dst[(row0 + rl) * H + f] = a.xc_src[(row0 + rl) * a.xc_ld + f];
        }
    for (int f0 = 0; f0 < H; f0 += 256) {
        const int f = f0 + tid;
        float acc[kGdRows];
#pragma unroll
        for (int rl = 0; rl < kGdRows; ++rl) acc[rl] = 0.f;
        for (int net = 0; net < 2; ++net) {
            __syncthreads();
            for (int i = tid; i < rows * P; i += 256) sm[i] = a.dqkv[net][row0 * P + i];
            __syncthreads();
            if (f < H) {
                for (int c = 0; c < P; ++c) {
                    const float w = c < a.nq ? a.Wq[net][(int64_t)f * a.nq + c]
                                  : c < 2 * a.nq ? a.Wk[net][(int64_t)f * a.nq + (c - a.nq)]
                                                 : a.Wv[net][(int64_t)f * a.NV + (c - 2 * a.nq)];
#pragma unroll
                    for (int rl = 0; rl < kGdRows; ++rl) acc[rl] += sm[rl * P + c] * w;
                }
            }
        }
        if (f < H)
            for (int rl = 0; rl < rows; ++rl) {
                const int64_t r = row0 + rl;
                a.g[r * a.ldg + f] += acc[rl] + a.dh0[0][r * a.in0 + f] + a.dh0[1][r * a.in0 + f];
            }
    }
}

template <int KG, int VT, int ST>
static size_t graph_bwd_lds_bytes() {
    constexpr int CH = 16 * ST;
    return ((size_t)16 * (KG + VT) * (CH + 4) + 3 * (size_t)CH) * sizeof(float);
}

int launch_attn_graph_backward(const GnfAttn* const* at, int64_t n, int32_t H, int32_t in0, const int32_t* node_offsets,
                               int64_t n_graphs, const float* const* qkv, const float* const* dagg, int64_t dagg_ld,
                               const float* const* agg, int64_t agg_ld, float* const* stats, float* const* dqkv,
                               const float* const* dh0, float* g_cond, int64_t ldg, const float* xc_src, int64_t xc_ld,
                               float* xc_dst, hipStream_t st) {
    if (n == 0) return GNF_OK;
    if (!node_offsets || n_graphs < 1 || n_graphs > INT32_MAX - 1) {
        set_error("graph-scope attention backward needs node_offsets of n_graphs >= 1 graphs");
        return GNF_EINVAL;
    }
    const GnfAttn* a0 = at[0];
    GraphAttnBwdArgs a;
    for (int q = 0; q < 2; ++q)
        a.qkv[q] = qkv[q], a.dagg[q] = dagg[q], a.agg[q] = agg[q], a.stats[q] = stats[q], a.dqkv[q] = dqkv[q];
    a.dagg_ld = dagg_ld, a.agg_ld = agg_ld;
    a.win = GraphAttnWin{node_offsets, (int32_t)n_graphs, (int32_t)n};
    a.nh = a0->num_heads, a.kq = a0->kq_dim, a.v = a0->v_dim;
    a.scale = a0->kq_dim_division ? 1.f / sqrtf((float)a0->kq_dim) : 1.f;
    const dim3 grid((unsigned)((n + kGbRows - 1) / kGbRows), 2);
    auto go = [&](auto kr, auto kk, size_t lds) -> int {
        hipLaunchKernelGGL(kr, grid, dim3(256), lds, st, a);
        GNF_LAUNCH_CHECK("k_attn_graph_bwd_rows");
        hipLaunchKernelGGL(kk, grid, dim3(256), lds, st, a);
        GNF_LAUNCH_CHECK("k_attn_graph_bwd_keys");
        return GNF_OK;
    };
    int rc;
    if (a.kq <= 16 && a.v <= 16) {
        rc = go(k_attn_graph_bwd_rows<1, 1, 8>, k_attn_graph_bwd_keys<1, 1, 8>, graph_bwd_lds_bytes<1, 1, 8>());
    } else if (a.kq <= 64 && a.v <= 64) {
        GNF_ONCE_PER_DEVICE(
            GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_graph_bwd_rows<4, 4, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_graph_bwd_keys<4, 4, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)));
        rc = go(k_attn_graph_bwd_rows<4, 4, 8>, k_attn_graph_bwd_keys<4, 4, 8>, graph_bwd_lds_bytes<4, 4, 8>());
    } else {
        GNF_ONCE_PER_DEVICE(
            GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_graph_bwd_rows<16, 16, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_graph_bwd_keys<16, 16, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)));
        rc = go(k_attn_graph_bwd_rows<16, 16, 4>, k_attn_graph_bwd_keys<16, 16, 4>, graph_bwd_lds_bytes<16, 16, 4>());
    }
    if (rc) return rc;
    GraphAttnDxArgs d;
    for (int q = 0; q < 2; ++q)
        d.dqkv[q] = dqkv[q], d.Wq[q] = at[q]->Wq, d.Wk[q] = at[q]->Wk, d.Wv[q] = at[q]->Wv, d.dh0[q] = dh0[q];
    d.g = g_cond, d.ldg = ldg;
    d.xc_src = xc_src, d.xc_ld = xc_ld, d.xc_dst = xc_dst;
    d.n = (int32_t)n, d.H = H, d.nq = a.nh * a.kq, d.NV = a.nh * a.v, d.in0 = in0;
    const size_t lds = (size_t)kGdRows * (2 * d.nq + d.NV) * sizeof(float);   // <= 16 x 768 floats inside the limit
    GNF_ONCE_PER_DEVICE(GNF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_graph_bwd_dx),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)));
    hipLaunchKernelGGL(k_attn_graph_bwd_dx, dim3((unsigned)((n + kGdRows - 1) / kGdRows)), dim3(256), lds, st, d);
    GNF_LAUNCH_CHECK("k_attn_graph_bwd_dx");
    return GNF_OK;
}

}  // namespace gnf
