// The encoder's backward pass (include/gnf_timestep_gnn_train.h): dL/d(parameters) and dL/dx of TimestepGNN (gnn.py:183-235)
// from dL/d out and the stash the training forward (gnf_timestep_gnn.hip) left.  The header states the mathematics operation
// by operation; this file is the walk and its kernels.
//
// One net per module call, on the building blocks the rest of the library runs (declared in gnf_common.h):
//   launch_mlp_hidden       the hidden layers again through the layered path's own run_mlps (gnf_layered.hip): the kernels the
//                           forward ran on the same operands, so the activation masks are the forward's, bit for bit
//   launch_linear_dx_one    dX = (dY W^T) * act'(h) on the generic matrix-core GEMM tile (gnf_train.hip, one job)
//   launch_weight_grad_one  dW = h^T dY and db = colsum dY as that tile's slab GEMM over a fixed number of row chunks (the
//                           column sums ride along) and k_reduce_grouped, which adds the slabs in chunk order (onto the
//                           gradient for a shared net's later uses)
//   k_enc_agg_bwd (here)    dL/dh_0 back through combine / aggregate along the sender-grouped CSR, written (not accumulated)
// The norm stage's backward is two launches per timestep, mirroring the forward's k_bn_stats + k_snt_norm:
//   k_enc_norm_bwd_reduce   a workgroup per chunk of rows.  With a layer norm: a wave per row, lanes along the features, does
//                           the row backward (rows re-read from L1, any width) and leaves the row's (mean, rstd); then the
//                           workgroup turns to columns and accumulates sum G, sum G u^ (batch norm) and sum G a^, sum G
//                           (layer norm) of its rows in fp64: one partial row [D][4] per workgroup
//   k_enc_norm_bwd_apply    every workgroup re-reduces the partial rows in order, keeps four constants per column in LDS and
//                           writes du for its sixteen rows; workgroup 0 writes dgamma / dbeta of both norms
// Nothing here uses an atomic: every sum has one owner and a fixed order.
#include <cstddef>
#include <cstring>

#include "gnf_common.h"

namespace gnf {

static constexpr int kEncParts = 128;      // most partial rows of the norm stage's backward (the workspace reserves them)
static constexpr int kEncPartMinRows = 32; // rows a partial covers at least
static constexpr int kEncDwChunks = 16;    // most row chunks (slabs) of a weight gradient
static constexpr int kEncDwAlign = 32;     // a chunk is whole k-steps of the generic GEMM tile
static constexpr size_t kEncSlabFloats = (size_t)16 << 20;   // ... and the most slab floats (64 MiB)

// g[u, f] = base + sum over edges u -> r (row u of the sender-grouped CSR, in edge order) of dh[r, c0 + f] * w(r)
//   agg combine: base = eps * dh[u, f], c0 = 0;  concat: base = dh[u, f], c0 = H;  w(r) = 1 / max(indeg(r), 1) with rowptr (the
//   receiver-grouped CSR's: the mean aggregator), else 1
__global__ __launch_bounds__(256) void k_enc_agg_bwd(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                                                     const int32_t* __restrict__ rowptr, int64_t n, const float* __restrict__ dh,
                                                     int in0, int H, int concat, float eps, float* __restrict__ g) {
    const int64_t total = n * H;
    const int c0 = concat ? H : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t u = i / H;
        const int f = (int)(i - u * H);
        float acc = 0.f;
        const int beg = rowptr_t[u], end = rowptr_t[u + 1];
        for (int e = beg; e < end; ++e) {
            const int64_t r = col_t[e];
            float w = 1.f;
            if (rowptr) {
                const int dg = rowptr[r + 1] - rowptr[r];
                w = 1.f / (float)(dg > 1 ? dg : 1);
            }
            acc += dh[r * in0 + c0 + f] * w;
        }
        const float own = dh[u * in0 + f];
        g[i] = (concat ? own : own * eps) + acc;
    }
}

// out[r, f] = g[r, f] (+ res[r, f])
__global__ __launch_bounds__(256) void k_enc_finish(const float* __restrict__ g, int64_t ldg, const float* __restrict__ res,
                                                    int64_t ldr, float* __restrict__ out, int64_t ldo, int64_t n, int D) {
    const int64_t total = n * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / D;
        const int f = (int)(i - r * D);
        float v = g[r * ldg + f];
        if (res) v += res[r * ldr + f];
        out[r * ldo + f] = v;
    }
}

// ---- the norm stage, backwards ------------------------------------------------------------------------------------------------
struct NormBwdArgs {
    const float* g;      // dL/d(the norm stage's output) [n, D], dense
    const float* u;      // the rows that entered the timestep [n, D], leading dimension ldu
    int64_t ldu;
    int64_t n;
    int32_t D;
    int32_t rows_per_part;
    int32_t nparts;
    // batch norm (bn_gamma == NULL: none): the stashed batch moments
    const float* mean;
    const float* var;
    const float* bn_gamma;
    const float* bn_beta;
    float eps;
    // layer norm (ln_gamma == NULL: none)
    const float* ln_gamma;
    float* gmid;         // with a layer norm: dL/d(its input) [n, D], dense (the reduce pass writes it)
    float* rowstat;      // ... and [n][2]: the row's mean and 1 / sqrt(var + GNF_LN_EPS)
    double* part;        // [nparts][D][4]: sum G_bn, sum G_bn u^, sum G a^, sum G   (G_bn = gmid with a layer norm, else g)
    float* gout;         // apply pass: du [n, D], dense
    float* d_bn_gamma;   // apply pass, workgroup 0
    float* d_bn_beta;
    float* d_ln_gamma;
    float* d_ln_beta;
};

// the layer norm's input at (r, c): the batch norm's output, formed as the forward forms it, or the timestep's input rows
static __device__ __forceinline__ float ln_input(const NormBwdArgs& a, float uv, int c) {
    if (!a.bn_gamma) return uv;
    const float iv = (1.f / sqrtf(a.var[c] + a.eps)) * a.bn_gamma[c];
    return fmaf(uv, iv, a.bn_beta[c] - a.mean[c] * iv);
}

// q = G * gamma as one rounded product in every pass over a row: were the product contracted into the subtraction of its own
// row mean, a row of one feature would keep the product's rounding error, times 1 / sqrt(GNF_LN_EPS), instead of exactly 0
static __device__ __forceinline__ float mul_rounded(float x, float y) {
#pragma clang fp contract(off)
    const float p = x * y;
    return p;
}

__global__ __launch_bounds__(256) void k_enc_norm_bwd_reduce(const NormBwdArgs a) {
    __shared__ double sh[4][256];
    const int D = a.D, tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_part;
    const int64_t r1 = r0 + a.rows_per_part < a.n ? r0 + a.rows_per_part : a.n;
    if (a.ln_gamma) {
        const int lane = tid & 63, wave = tid >> 6;
        const float inv_d = 1.f / (float)D;
        for (int64_t r = r0 + wave; r < r1; r += 4) {
            const float* ur = a.u + r * a.ldu;
            const float* gr = a.g + r * D;
            float sum = 0.f;
            for (int f = lane; f < D; f += 64) sum += ln_input(a, ur[f], f);
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
            const float mean = sum * inv_d;
            float sq = 0.f;
            for (int f = lane; f < D; f += 64) {
                const float d = ln_input(a, ur[f], f) - mean;
                sq = fmaf(d, d, sq);
            }
            for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
            const float rstd = 1.f / sqrtf(sq * inv_d + GNF_LN_EPS);
            float sq1 = 0.f, sqa = 0.f;
            for (int f = lane; f < D; f += 64) {
                const float q = mul_rounded(gr[f], a.ln_gamma[f]);
                const float ah = (ln_input(a, ur[f], f) - mean) * rstd;
                sq1 += q;
                sqa = fmaf(q, ah, sqa);
            }
            for (int off = 32; off > 0; off >>= 1) {
                sq1 += __shfl_xor(sq1, off, 64);
                sqa += __shfl_xor(sqa, off, 64);
            }
            const float mq = sq1 * inv_d, mqa = sqa * inv_d;
            for (int f = lane; f < D; f += 64) {
                const float q = mul_rounded(gr[f], a.ln_gamma[f]);
                const float ah = (ln_input(a, ur[f], f) - mean) * rstd;
                a.gmid[r * D + f] = (q - mq - ah * mqa) * rstd;
            }
            if (lane == 0) {
                a.rowstat[2 * r] = mean;
                a.rowstat[2 * r + 1] = rstd;
            }
        }
        __syncthreads();   // this workgroup's gmid rows and row statistics are read back below
    }
    // columns: cols lanes along the features, rl row lanes; the row lanes' sums are added in order
    int cols = 1;
    while (cols < D && cols < 256) cols <<= 1;
    const int rl = 256 / cols, cl = tid % cols, rr = tid / cols;
    for (int c0 = 0; c0 < D; c0 += cols) {
        const int c = c0 + cl;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if (c < D) {
            float mean_c = 0.f, rs_c = 0.f;
            if (a.bn_gamma) mean_c = a.mean[c], rs_c = 1.f / sqrtf(a.var[c] + a.eps);
            for (int64_t r = r0 + rr; r < r1; r += rl) {
                const float gv = a.g[r * D + c];
                const float uv = a.u[r * a.ldu + c];
                float gb = gv;
                if (a.ln_gamma) {
                    const float ah = (ln_input(a, uv, c) - a.rowstat[2 * r]) * a.rowstat[2 * r + 1];
                    s[2] += (double)gv * (double)ah;
                    s[3] += (double)gv;
                    gb = a.gmid[r * D + c];
                }
                if (a.bn_gamma) {
                    const float uh = (uv - mean_c) * rs_c;
                    s[0] += (double)gb;
                    s[1] += (double)gb * (double)uh;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) sh[q][tid] = s[q];
        __syncthreads();
        if (rr == 0 && c < D) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double tot = 0.0;
                for (int k = 0; k < rl; ++k) tot += sh[q][k * cols + cl];
                a.part[((int64_t)blockIdx.x * D + c) * 4 + q] = tot;
            }
        }
        __syncthreads();
    }
}

static constexpr int kEncApplyRows = 16;

// gridDim.x == 1 and no batch norm: only the layer norm's dgamma / dbeta are written (its du left the reduce pass)
__global__ __launch_bounds__(256) void k_enc_norm_bwd_apply(const NormBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ks[];   // k1[D] | k2[D] | k3[D] | mean[D]   (batch norm only)
    const int D = a.D, tid = threadIdx.x;
    float* k1 = ks;
    float* k2 = ks + D;
    float* k3 = ks + 2 * D;
    float* km = ks + 3 * D;
    const double inv_n = 1.0 / (double)a.n;
    for (int c = tid; c < D; c += 256) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < a.nparts; ++b) {
            const double* p = a.part + ((int64_t)b * D + c) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += p[q];
        }
        if (a.bn_gamma) {
            const float rs = 1.f / sqrtf(a.var[c] + a.eps);
            k1[c] = a.bn_gamma[c] * rs;
            k2[c] = (float)(s[0] * inv_n);
            k3[c] = (float)((double)rs * s[1] * inv_n);
            km[c] = a.mean[c];
        }
        if (blockIdx.x == 0) {
            if (a.bn_gamma) {
                a.d_bn_beta[c] = (float)s[0];
                a.d_bn_gamma[c] = (float)s[1];
            }
            if (a.ln_gamma) {
                a.d_ln_gamma[c] = (float)s[2];
                a.d_ln_beta[c] = (float)s[3];
            }
        }
    }
    if (!a.bn_gamma) return;
    __syncthreads();
    const float* gsrc = a.ln_gamma ? a.gmid : a.g;
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kEncApplyRows;
    const int64_t r1 = r0 + kEncApplyRows < a.n ? r0 + kEncApplyRows : a.n;
    for (int64_t r = r0 + wave; r < r1; r += 4)
        for (int f = lane; f < D; f += 64) {
            const float uc = a.u[r * a.ldu + f] - km[f];
            a.gout[r * D + f] = k1[f] * (gsrc[r * D + f] - k2[f] - uc * k3[f]);
        }
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------
static inline size_t al64(size_t v) { return (v + 63) / 64 * 64; }

struct EncBwdPlan {
    int K, in0, wmax;
    int chunks;            // row chunks of a weight gradient
    int64_t rows_per_chunk;
    size_t part_bytes;     // 256-aligned
    size_t gbuf;           // floats of one [n, D] gradient buffer
    size_t rowstat;        // floats (layer norm only)
    int ldh;               // row stride of h_1 .. h_{K-1} (hidden_max, as in the forward's scratch)
    size_t h_off[GNF_MAX_LAYERS];   // floats from the start of the h region: h_0 [n, in0], h_1 .. h_{K-1} [n, ldh]
    size_t h_total;
    size_t dp;             // floats of one dP buffer
    size_t wslab, bslab;   // floats
    size_t total_bytes;
};

static EncBwdPlan enc_bwd_plan(int64_t n, int32_t D, const GnfTimestepGnn* g) {
    EncBwdPlan p;
    memset(&p, 0, sizeof(p));
    const GnfMlp* m = &g->nets[0];
    p.K = m->num_layers;
    p.in0 = m->dims[0];
    size_t max_io = 0, max_o = 0;
    for (int j = 0; j < p.K; ++j) {
        if (m->dims[j] > p.wmax) p.wmax = m->dims[j];
        const size_t io = (size_t)m->dims[j] * (size_t)m->dims[j + 1];
        if (io > max_io) max_io = io;
        if ((size_t)m->dims[j + 1] > max_o) max_o = m->dims[j + 1];
    }
    p.ldh = hidden_max(m);
    for (int j = 0; j < p.K; ++j) {
        p.h_off[j] = p.h_total;
        p.h_total += al64((size_t)n * (size_t)(j == 0 ? p.in0 : p.ldh));
    }
    int64_t chunks = (n + 255) / 256;
    if (chunks > kEncDwChunks) chunks = kEncDwChunks;
    while (chunks > 1 && (size_t)chunks * max_io > kEncSlabFloats) --chunks;
    if (chunks < 1) chunks = 1;
    p.chunks = (int)chunks;
    p.rows_per_chunk = ((n + chunks - 1) / chunks + kEncDwAlign - 1) / kEncDwAlign * kEncDwAlign;
    if (p.rows_per_chunk < kEncDwAlign) p.rows_per_chunk = kEncDwAlign;
    const bool norms = g->bns || g->lns;
    const size_t pb = norms ? (size_t)kEncParts * (size_t)D * 4 * sizeof(double) : 0;
    p.part_bytes = (pb + 255) / 256 * 256;
    p.gbuf = al64((size_t)n * (size_t)D);
    p.rowstat = g->lns ? al64((size_t)n * 2) : 0;
    p.dp = al64((size_t)n * (size_t)p.wmax);
    p.wslab = al64((size_t)p.chunks * max_io);
    p.bslab = al64((size_t)p.chunks * max_o);
    p.total_bytes = p.part_bytes + (3 * p.gbuf + p.rowstat + p.h_total + 2 * p.dp + p.wslab + p.bslab) * sizeof(float);
    return p;
}

struct EncBwdBuffers {
    double* part;
    float* gbuf[3];
    float* rowstat;
    float* h;
    float* dp[2];
    float* wslab;
    float* bslab;
};

static EncBwdBuffers enc_bwd_buffers(const EncBwdPlan& p, void* ws) {
    EncBwdBuffers b;
    b.part = (double*)ws;
    float* f = (float*)((char*)ws + p.part_bytes);
    for (int k = 0; k < 3; ++k) b.gbuf[k] = f, f += p.gbuf;
    b.rowstat = f, f += p.rowstat;
    b.h = f, f += p.h_total;
    for (int k = 0; k < 2; ++k) b.dp[k] = f, f += p.dp;
    b.wslab = f, f += p.wslab;
    b.bslab = f;
    return b;
}

// one GNN module call backwards: v [n, D] (leading dimension ldv) the rows that entered it, G [n, D] (ldG) dL/d(its output);
// writes dL/dv into gnew (dense) and the net's gradients into gm (accumulate: onto them)
static int module_backward(const GnfCsr* csr, const GnfCsr* csr_t, const GnfGnnSpec& gnn, const GnfMlp* m, const GnfMlp* gm,
                           const float* v, int64_t ldv, const float* G, int64_t ldG, float* gnew, int32_t D,
                           const EncBwdPlan& p, const EncBwdBuffers& b, int accumulate, hipStream_t st) {
    const int64_t n = csr->n_nodes;
    const int K = p.K;
    const int concat = gnn.combine == GNF_COMBINE_CONCAT ? 1 : 0;
    const int mean = gnn.agg == GNF_AGG_MEAN ? 1 : 0;
    int rc = launch_aggregate(csr->rowptr, csr->col, n, v, ldv, D, mean, concat, gnn.epsilon, b.h + p.h_off[0], p.in0, st);
    if (rc) return rc;
    if (K > 1) {   // the hidden layers again, as the forward ran them
        float* hidden[GNF_MAX_LAYERS] = {};
        for (int j = 1; j < K; ++j) hidden[j - 1] = b.h + p.h_off[j];
        rc = launch_mlp_hidden(m, b.h + p.h_off[0], p.in0, hidden, p.ldh, n, gnn, st);
        if (rc) return rc;
    }
    const int chunks = (int)((n + p.rows_per_chunk - 1) / p.rows_per_chunk);
    const float* dP = G;
    int64_t lddp = ldG;
    for (int j = K - 1; j >= 0; --j) {
        const int I = m->dims[j], O = m->dims[j + 1];
        const float* hj = b.h + p.h_off[j];
        const int64_t ldhj = j == 0 ? p.in0 : p.ldh;
        // dW_j = h_j^T dP, db_j = colsum dP: slabs over the row chunks, summed in chunk order
        rc = launch_weight_grad_one(hj, ldhj, dP, lddp, n, I, O, chunks, p.rows_per_chunk, b.wslab, b.bslab, (float*)gm->W[j],
                                    (float*)gm->b[j], accumulate, st);
        if (rc) return rc;
        // dP_j = (dP W_j^T) * act'(h_j)   (j = 0: dL/dh_0, no mask)
        float* dst = dP == b.dp[0] ? b.dp[1] : b.dp[0];
        rc = launch_linear_dx_one(dP, lddp, m->W[j], dst, I, j >= 1 ? hj : nullptr, ldhj, n, I, O, gnn.activation, gnn.alpha, st);
        if (rc) return rc;
        dP = dst, lddp = I;
    }
    int64_t blocks = (n * D + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_enc_agg_bwd, dim3((unsigned)blocks), dim3(256), 0, st, csr_t->rowptr, csr_t->col,
                       mean ? csr->rowptr : (const int32_t*)nullptr, n, dP, p.in0, D, concat, gnn.epsilon, gnew);
    GNF_LAUNCH_CHECK("k_enc_agg_bwd");
    return GNF_OK;
}

static float* other_buffer(const EncBwdBuffers& b, const float* x, const float* y) {
    for (int k = 0; k < 3; ++k)
        if (b.gbuf[k] != x && b.gbuf[k] != y) return b.gbuf[k];
    return nullptr;
}

static int zero_gradients(const GnfTimestepGnn* g, const GnfTimestepGnn* grad, int32_t D, hipStream_t st) {
    const int n_nets = g->weight_sharing ? 1 : g->num_timesteps;
    for (int q = 0; q < n_nets; ++q) {
        const GnfMlp* m = &g->nets[q];
        for (int j = 0; j < m->num_layers; ++j) {
            GNF_HIP_TRY(hipMemsetAsync((void*)grad->nets[q].W[j], 0, (size_t)m->dims[j] * m->dims[j + 1] * sizeof(float), st));
            GNF_HIP_TRY(hipMemsetAsync((void*)grad->nets[q].b[j], 0, (size_t)m->dims[j + 1] * sizeof(float), st));
        }
    }
    for (int i = 0; i < g->num_timesteps; ++i) {
        if (g->bns) {
            GNF_HIP_TRY(hipMemsetAsync((void*)grad->bns[i].gamma, 0, (size_t)D * sizeof(float), st));
            GNF_HIP_TRY(hipMemsetAsync((void*)grad->bns[i].beta, 0, (size_t)D * sizeof(float), st));
        }
        if (g->lns) {
            GNF_HIP_TRY(hipMemsetAsync((void*)grad->lns[i].gamma, 0, (size_t)D * sizeof(float), st));
            GNF_HIP_TRY(hipMemsetAsync((void*)grad->lns[i].beta, 0, (size_t)D * sizeof(float), st));
        }
    }
    return GNF_OK;
}

static int validate_grad(const GnfTimestepGnn* g, const GnfTimestepGnn* grad, const char* what) {
    if (!grad || !grad->nets) {
        set_error("%s: null grad / grad->nets", what);
        return GNF_EINVAL;
    }
    if (grad->num_timesteps != g->num_timesteps || (grad->weight_sharing != 0) != (g->weight_sharing != 0) ||
        (grad->bns != nullptr) != (g->bns != nullptr) || (grad->lns != nullptr) != (g->lns != nullptr)) {
        set_error("%s: grad has another shape than g (num_timesteps %d vs %d, weight_sharing %d vs %d, bns %d vs %d, lns %d vs %d)", what,
                  grad->num_timesteps, g->num_timesteps, grad->weight_sharing, g->weight_sharing, grad->bns != nullptr,
                  g->bns != nullptr, grad->lns != nullptr, g->lns != nullptr);
        return GNF_EINVAL;
    }
    const int n_nets = g->weight_sharing ? 1 : g->num_timesteps;
    for (int q = 0; q < n_nets; ++q) {
        const GnfMlp *m = &g->nets[q], *gm = &grad->nets[q];
        if (gm->num_layers != m->num_layers || memcmp(gm->dims, m->dims, sizeof(int32_t) * (m->num_layers + 1))) {
            set_error("%s: grad net %d has other layer widths than g's", what, q);
            return GNF_EINVAL;
        }
        for (int j = 0; j < m->num_layers; ++j)
            if (!gm->W[j] || !gm->b[j]) {
                set_error("%s: grad net %d layer %d has a null W / b", what, q, j);
                return GNF_EINVAL;
            }
    }
    for (int i = 0; i < g->num_timesteps; ++i) {
        if (g->bns && (!grad->bns[i].gamma || !grad->bns[i].beta)) {
            set_error("%s: grad batch norm %d has a null gamma / beta", what, i);
            return GNF_EINVAL;
        }
        if (g->lns && (!grad->lns[i].gamma || !grad->lns[i].beta)) {
            set_error("%s: grad layer norm %d has a null gamma / beta", what, i);
            return GNF_EINVAL;
        }
    }
    return GNF_OK;
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_timestep_gnn_backward_workspace_bytes(int64_t n_nodes, int32_t D, const GnfTimestepGnn* g) {
    if (n_nodes < 0 || n_nodes > kEncMaxNodes || D < 1 || !g || !g->nets || g->num_timesteps < 1) return 0;
    const GnfMlp* m = &g->nets[0];
    if (m->attn || m->num_layers < 1 || m->num_layers > GNF_MAX_LAYERS) return 0;
    return enc_bwd_plan(n_nodes, D, g).total_bytes;
}

int gnf_timestep_gnn_backward_f32(const GnfCsr* csr, const GnfCsr* csr_t, const GnfTimestepGnn* g, const GnfTimestepGnn* grad,
                                  const float* x, int64_t ldx, const float* g_out, int64_t ldg, float* g_x, int64_t ldgx,
                                  int32_t D, const void* stash, size_t stash_bytes, void* ws, size_t ws_bytes,
                                  gnf_stream_t stream) {
    const char* what = "gnf_timestep_gnn_backward_f32";
    int rc = validate_encoder(csr, g, ldx, D, D, what);
    if (rc) return rc;
    rc = validate_encoder_train(g, what);
    if (rc) return rc;
    if (!csr_t || !csr_t->rowptr || (!csr_t->col && csr_t->n_edges > 0) || csr_t->n_nodes != csr->n_nodes ||
        csr_t->n_edges != csr->n_edges) {
        set_error("%s: csr_t (the edges grouped by sender) is null, has null arrays or another size than csr", what);
        return GNF_EINVAL;
    }
    rc = validate_grad(g, grad, what);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = csr->n_nodes;
    if (n == 0) return zero_gradients(g, grad, D, st);
    if (n > kEncMaxNodes) {
        set_error("%s: n_nodes=%lld (at most %lld)", what, (long long)n, (long long)kEncMaxNodes);
        return GNF_EUNSUPPORTED;
    }
    if (!x || !g_out || !stash || !ws) {
        set_error("%s: null x / g_out / stash / ws", what);
        return GNF_EINVAL;
    }
    if (ldg < D || (g_x && ldgx < D)) {
        set_error("%s: ldg=%lld ldgx=%lld (need >= D=%d)", what, (long long)ldg, (long long)ldgx, D);
        return GNF_ESHAPE;
    }
    if (g_x) {
        const uintptr_t a0 = (uintptr_t)g_out, a1 = a0 + ((size_t)(n - 1) * (size_t)ldg + (size_t)D) * sizeof(float);
        const uintptr_t b0 = (uintptr_t)g_x, b1 = b0 + ((size_t)(n - 1) * (size_t)ldgx + (size_t)D) * sizeof(float);
        if (a0 < b1 && b0 < a1) {
            set_error("%s: g_x and g_out overlap (g_out is never written)", what);
            return GNF_EINVAL;
        }
    }
    if ((uintptr_t)ws % sizeof(double) || (uintptr_t)stash % sizeof(double)) {
        set_error("%s: ws and stash must be 8-byte aligned", what);
        return GNF_EINVAL;
    }
    const EncoderStash sp = encoder_stash(n, D, g);
    if (stash_bytes < sp.total_bytes) {
        set_error("%s: stash %zu < %zu bytes", what, stash_bytes, sp.total_bytes);
        return GNF_EWORKSPACE;
    }
    const EncBwdPlan p = enc_bwd_plan(n, D, g);
    if (ws_bytes < p.total_bytes) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, p.total_bytes);
        return GNF_EWORKSPACE;
    }
    const EncBwdBuffers b = enc_bwd_buffers(p, ws);
    const float* sf = (const float*)stash;
    const int T = g->num_timesteps;
    // dL/d out as dense rows of the workspace: every GEMM operand of the walk is then a 256-byte aligned buffer of this call
    rc = launch_copy_rows(g_out, ldg, b.gbuf[2], D, n, D, st);
    if (rc) return rc;
    const float* G = b.gbuf[2];
    int64_t ldG = D;
    for (int i = T - 1; i >= 0; --i) {
        const float* uin = i == 0 ? x : sf + (size_t)(i - 1) * sp.buf_floats;   // the rows that entered the timestep
        const int64_t ldu = i == 0 ? ldx : D;
        const float* v = sp.norms ? sf + sp.v_off + (size_t)i * sp.buf_floats : uin;
        const int64_t ldv = sp.norms ? D : ldu;
        const int q = g->weight_sharing ? 0 : i;
        float* gnew = other_buffer(b, G, nullptr);
        rc = module_backward(csr, csr_t, g->gnn, &g->nets[q], &grad->nets[q], v, ldv, G, ldG, gnew, D, p, b,
                             g->weight_sharing && i != T - 1, st);
        if (rc) return rc;
        G = gnew, ldG = D;
        if (!sp.norms) continue;
        NormBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.g = G, a.u = uin, a.ldu = ldu, a.n = n, a.D = D;
        int64_t rpp = (n + kEncParts - 1) / kEncParts;
        if (rpp < kEncPartMinRows) rpp = kEncPartMinRows;
        a.rows_per_part = (int32_t)rpp;
        a.nparts = (int32_t)((n + rpp - 1) / rpp);
        if (g->bns) {
            a.mean = sf + sp.mom_off + (size_t)(2 * i) * sp.dpad;
            a.var = a.mean + sp.dpad;
            a.bn_gamma = g->bns[i].gamma, a.bn_beta = g->bns[i].beta, a.eps = g->bn_eps;
            a.d_bn_gamma = (float*)grad->bns[i].gamma, a.d_bn_beta = (float*)grad->bns[i].beta;
        }
        if (g->lns) {
            a.ln_gamma = g->lns[i].gamma;
            a.gmid = other_buffer(b, G, nullptr);
            a.rowstat = b.rowstat;
            a.d_ln_gamma = (float*)grad->lns[i].gamma, a.d_ln_beta = (float*)grad->lns[i].beta;
        }
        a.part = b.part;
        a.gout = g->bns ? other_buffer(b, G, a.gmid) : nullptr;
        hipLaunchKernelGGL(k_enc_norm_bwd_reduce, dim3((unsigned)a.nparts), dim3(256), 0, st, a);
        GNF_LAUNCH_CHECK("k_enc_norm_bwd_reduce");
        const int64_t blocks = g->bns ? (n + kEncApplyRows - 1) / kEncApplyRows : 1;
        hipLaunchKernelGGL(k_enc_norm_bwd_apply, dim3((unsigned)blocks), dim3(256), g->bns ? (size_t)4 * D * sizeof(float) : 0, st, a);
        GNF_LAUNCH_CHECK("k_enc_norm_bwd_apply");
        G = g->bns ? a.gout : a.gmid;
    }
    if (g_x) {
        int64_t blocks = (n * D + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(k_enc_finish, dim3((unsigned)blocks), dim3(256), 0, st, G, ldG, g->residual ? g_out : (const float*)nullptr,
                           ldg, g_x, ldgx, n, D);
        GNF_LAUNCH_CHECK("k_enc_finish");
    }
    return GNF_OK;
}

}  // extern "C"
