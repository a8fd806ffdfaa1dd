// The encoder's forward pass (include/gnf_timestep_gnn.h): TimestepGNN (gnn.py:183-235) - T GNN module calls in a row, each
// optionally behind snt.BatchNorm(scale=True) (gnn.py:210-213, 220-225) and / or snt.LayerNorm() (gnn.py:214-215, 226-228),
// and the final residual (gnn.py:233-234).
//
// The module calls are launch_gnn_layered - what gnf_gnn_apply_f32 runs, so their bits are its bits.  New here is the norm
// stage: launch_bn_stats (gnf_bn.hip) leaves the batch's fp64 column sums as a few partial rows, k_snt_norm re-reduces them
// in fixed order in every workgroup, forms inv / shift per column in LDS and writes the normalised rows OUT OF PLACE (the
// caller's x is never written: the residual needs it); with a LayerNorm on the same timestep it is applied to the rows
// before they are stored - one pass over the rows, not two.  Workgroup 0 writes the batch moments and, in training mode, the
// moving-average update.
//
// Semantics restated from Sonnet 1.x batch_norm.py / layer_norm.py (third party, absent here: UNPINNED):
//   snt.BatchNorm(scale=True)(x, is_training, test_local_stats): use_batch_stats = is_training | test_local_stats;
//     mean, variance = tf.nn.moments(x, [0]) (biased) when use_batch_stats, else the moving statistics;
//     when is_training: assign_moving_average(moving, batch, decay_rate, zero_debias=False) for both, i.e.
//       moving -= (moving - batch) * (1 - decay_rate), the variance being the SAME biased batch variance;
//     tf.nn.batch_normalization(x, mean, variance, beta, gamma, eps): inv = rsqrt(variance + eps) * gamma,
//       y = x * inv + (beta - mean * inv);  defaults decay_rate = 0.999, eps = 1e-3, gamma ones, beta zeros,
//       moving_mean zeros, moving_variance ones.
//   snt.LayerNorm(): as k_layer_norm (gnf_layered.hip).
#include <cstddef>
#include <cstring>

#include "gnf_common.h"

// the signature check below compares the eight int32 geometry members of GnfAttn (num_heads .. layer_norm) as one block
static_assert(offsetof(GnfAttn, Wq) == 8 * sizeof(int32_t), "GnfAttn's geometry members are its first eight int32");
static_assert(sizeof(GnfSntBatchNorm) == 48 && sizeof(GnfRowNorm) == 16 && sizeof(GnfTimestepGnn) == 80,
              "the ctypes mirrors (_abi.py) assume these sizes");

namespace gnf {

static constexpr int kSntRows = 16;       // rows per workgroup of the normalising pass (four waves, one row each at a time)
// partial rows launch_bn_stats leaves at most: bn_blocks cuts n rows into chunks of max(ceil(n / 16), 32) rows, so it never
// yields more than 16 for any n (the workspace reserves exactly that many)
static constexpr int kSntPartRows = 16;
// (kSntMaxWidth, the widest batch norm - inv | shift of every column in LDS, 32 KiB - is in gnf_common.h: the backward shares it)

struct SntNormArgs {
    const float* x;   // [n, D], leading dimension ldx: never written
    int64_t ldx;
    float* y;         // [n, D], leading dimension ldy
    int64_t ldy;
    int64_t n;
    int32_t D;
    const double* part;   // [nparts][D][2] column sums / sums of squares; nparts == 0: the moving statistics normalise
    int32_t nparts;
    const float* gamma;
    const float* beta;
    float* moving_mean;
    float* moving_var;
    float* batch_mean;    // nullable
    float* batch_var;
    float eps;
    float one_minus_decay;
    int32_t update_moving;
    const float* ln_gamma;   // NULL: no layer norm behind the batch norm
    const float* ln_beta;
};

// The scalar arithmetic the header states operation by operation.  hipcc contracts a * b + c into one fma by default (and its
// __fmul_rn / __fsub_rn are plain operators that inline into the same expression): contraction is switched off for these two.
// moving -= (moving - batch) * (1 - decay): three separately rounded fp32 operations (assign_moving_average's sub, mul, sub)
static __device__ __forceinline__ float moving_average(float moving, float batch, float one_minus_decay) {
#pragma clang fp contract(off)
    const float delta = (moving - batch) * one_minus_decay;
    return moving - delta;
}
// tf.nn.batch_normalization: inv = rsqrt(var + eps) * gamma, shift = beta - mean * inv
static __device__ __forceinline__ void snt_scale_shift(float mean, float var, float eps, float gamma, float beta, float* inv,
                                                       float* shift) {
#pragma clang fp contract(off)
    const float iv = (1.f / sqrtf(var + eps)) * gamma;
    const float mi = mean * iv;
    *inv = iv;
    *shift = beta - mi;
}

// One wave per row, lanes along the features.  A row of up to 256 features stays in four registers per lane between the
// layer norm's three passes; wider rows are read again (they sit in L1) and normalised again with the same fmaf.
__global__ __launch_bounds__(256) void k_snt_norm(const SntNormArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ss[];   // inv[D] | shift[D]
    const int D = a.D;
    float* inv = ss;
    float* shift = ss + D;
    const int tid = threadIdx.x;
    for (int c = tid; c < D; c += 256) {
        float mean, var;
        if (a.nparts > 0) {
            double s = 0.0, q = 0.0;
            for (int b0 = 0; b0 < a.nparts; b0 += 8) {   // eight partial pairs in flight, summed in order
                double ps[8], pq[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int b = b0 + k < a.nparts ? b0 + k : a.nparts - 1;
                    ps[k] = a.part[((int64_t)b * D + c) * 2 + 0];
                    pq[k] = a.part[((int64_t)b * D + c) * 2 + 1];
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (b0 + k < a.nparts) {
                        s += ps[k];
                        q += pq[k];
                    }
            }
            const double m = s / (double)a.n;
            double v = q / (double)a.n - m * m;   // biased (tf.nn.moments)
            if (v < 0.0) v = 0.0;
            mean = (float)m;
            var = (float)v;
            if (blockIdx.x == 0) {
                if (a.batch_mean) a.batch_mean[c] = mean;
                if (a.batch_var) a.batch_var[c] = var;
                if (a.update_moving) {
                    a.moving_mean[c] = moving_average(a.moving_mean[c], mean, a.one_minus_decay);
                    a.moving_var[c] = moving_average(a.moving_var[c], var, a.one_minus_decay);
                }
            }
        } else {
            mean = a.moving_mean[c];
            var = a.moving_var[c];
        }
        snt_scale_shift(mean, var, a.eps, a.gamma[c], a.beta[c], &inv[c], &shift[c]);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kSntRows;
    const int64_t r1 = r0 + kSntRows < a.n ? r0 + kSntRows : a.n;
    const bool in_regs = D <= 256;
    const float inv_d = 1.f / (float)D;
    for (int64_t r = r0 + wave; r < r1; r += 4) {
        const float* xr = a.x + r * a.ldx;
        float* yr = a.y + r * a.ldy;
        if (!a.ln_gamma) {
            for (int f = lane; f < D; f += 64) yr[f] = fmaf(xr[f], inv[f], shift[f]);
            continue;
        }
        float v[4];
        float sum = 0.f;
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int f = lane + 64 * k;
                v[k] = f < D ? fmaf(xr[f], inv[f], shift[f]) : 0.f;
                sum += v[k];   // (features past D add zeros: the order of the real terms is k_layer_norm's)
            }
        } else {
            for (int f = lane; f < D; f += 64) sum += fmaf(xr[f], inv[f], shift[f]);
        }
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        const float mean = sum * inv_d;
        float sq = 0.f;
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (lane + 64 * k < D) {
                    const float d = v[k] - mean;
                    sq = fmaf(d, d, sq);
                }
        } else {
            for (int f = lane; f < D; f += 64) {
                const float d = fmaf(xr[f], inv[f], shift[f]) - mean;
                sq = fmaf(d, d, sq);
            }
        }
        for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
        const float rstd = 1.f / sqrtf(sq * inv_d + GNF_LN_EPS);
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int f = lane + 64 * k;
                if (f < D) yr[f] = (v[k] - mean) * rstd * a.ln_gamma[f] + a.ln_beta[f];
            }
        } else {
            for (int f = lane; f < D; f += 64)
                yr[f] = (fmaf(xr[f], inv[f], shift[f]) - mean) * rstd * a.ln_gamma[f] + a.ln_beta[f];
        }
    }
}

// ---- workspace: [ fp64 moment partials | ping | pong | scratch of one module call ] ------------------------------------------
struct EncoderPlan {
    size_t part_bytes;     // 256-aligned
    size_t buf_floats;     // one [n, D] buffer, rounded up to 64 floats
    size_t scratch_floats;
    size_t total_bytes;
};

static EncoderPlan encoder_plan(int64_t n, int32_t D, const GnfTimestepGnn* g) {
    EncoderPlan p;
    const size_t pb = g->bns ? (size_t)kSntPartRows * (size_t)D * 2 * sizeof(double) : 0;
    p.part_bytes = (pb + 255) / 256 * 256;
    p.buf_floats = ((size_t)n * (size_t)D + 63) / 64 * 64;
    p.scratch_floats = plan_workspace(n, D, &g->nets[0], g->gnn.combine, 0).scratch_floats;
    p.total_bytes = p.part_bytes + (2 * p.buf_floats + p.scratch_floats) * sizeof(float);
    return p;
}

static bool uses_batch_stats(const GnfTimestepGnn* g) { return g->is_training || g->test_local_stats; }

int validate_encoder(const GnfCsr* csr, const GnfTimestepGnn* g, int64_t ldx, int64_t ldo, int32_t D, const char* what) {
    int rc = validate_csr(csr);
    if (rc) return rc;
    if (!g || !g->nets) {
        set_error("%s: null GnfTimestepGnn / nets", what);
        return GNF_EINVAL;
    }
    rc = validate_spec(&g->gnn);
    if (rc) return rc;
    const int T = g->num_timesteps;
    if (T < 1) {
        set_error("%s: num_timesteps=%d must be >= 1", what, T);
        return GNF_ESHAPE;
    }
    if (D < 1 || ldx < D || ldo < D) {
        set_error("%s: D=%d ldx=%lld ldo=%lld (need D >= 1, ldx >= D, ldo >= D)", what, D, (long long)ldx, (long long)ldo);
        return GNF_ESHAPE;
    }
    const int n_nets = g->weight_sharing ? 1 : T;
    const GnfMlp* m0 = &g->nets[0];
    for (int q = 0; q < n_nets; ++q) {
        const GnfMlp* m = &g->nets[q];
        rc = validate_mlp(m, what);
        if (rc) return rc;
        if (m->attn) {
            rc = validate_attn(m->attn, m, D, what);
            if (rc) return rc;
        }
        const int in0 = m->attn ? m->dims[0] : (g->gnn.combine == GNF_COMBINE_CONCAT ? 2 * D : D);
        if (m->dims[0] != in0 || m->dims[m->num_layers] != D) {
            set_error("%s: net %d maps %d -> %d but the encoder needs %d -> %d (D=%d, combine=%d)", what, q, m->dims[0],
                      m->dims[m->num_layers], in0, D, D, g->gnn.combine);
            return GNF_ESHAPE;
        }
        // one make_gnn_fn builds every net (gnn.py:206-209): one signature
        const GnfAttn *aq = m->attn, *a0 = m0->attn;
        if (m->num_layers != m0->num_layers || memcmp(m->dims, m0->dims, sizeof(int32_t) * (m0->num_layers + 1)) ||
            (aq != nullptr) != (a0 != nullptr) ||
            (aq && (memcmp(aq, a0, 8 * sizeof(int32_t)) || aq->scope != a0->scope || (aq->Wo == nullptr) != (a0->Wo == nullptr)))) {
            set_error("%s: net %d has another signature (layer widths / attention front-end) than net 0", what, q);
            return GNF_ESHAPE;
        }
    }
    rc = validate_node_offsets(csr, m0, what);
    if (rc) return rc;
    if (g->bns) {
        if (!(g->bn_eps > 0.f)) {
            set_error("%s: bn_eps must be > 0", what);
            return GNF_EINVAL;
        }
        if (g->is_training && !(g->bn_decay >= 0.f && g->bn_decay <= 1.f)) {
            set_error("%s: bn_decay=%g outside [0, 1]", what, (double)g->bn_decay);
            return GNF_EINVAL;
        }
        const bool need_moving = g->is_training || !g->test_local_stats;
        for (int i = 0; i < T; ++i) {
            const GnfSntBatchNorm* b = &g->bns[i];
            if (!b->gamma || !b->beta) {
                set_error("%s: batch norm %d has a null gamma / beta", what, i);
                return GNF_EINVAL;
            }
            if (need_moving && (!b->moving_mean || !b->moving_variance)) {
                set_error("%s: batch norm %d has null moving statistics (%s them)", what, i,
                          g->is_training ? "training updates" : "evaluation without test_local_stats reads");
                return GNF_EINVAL;
            }
        }
        if (D > kSntMaxWidth) {
            set_error("%s: batch norm over D=%d columns (at most %d)", what, D, kSntMaxWidth);
            return GNF_EUNSUPPORTED;
        }
    }
    if (g->lns)
        for (int i = 0; i < T; ++i)
            if (!g->lns[i].gamma || !g->lns[i].beta) {
                set_error("%s: layer norm %d has a null gamma / beta", what, i);
                return GNF_EINVAL;
            }
    return GNF_OK;
}

// keep_mean / keep_var (the training forward's stash, or NULL): where the batch moments go instead of bns[i].batch_mean /
// batch_variance, which then receive a copy
static int launch_snt_norm(const GnfTimestepGnn* g, int i, const float* x, int64_t ldx, float* y, int64_t n, int32_t D,
                           double* part, hipStream_t st, float* keep_mean = nullptr, float* keep_var = nullptr) {
    const GnfSntBatchNorm* b = &g->bns[i];
    SntNormArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x, a.ldx = ldx, a.y = y, a.ldy = D, a.n = n, a.D = D;
    if (uses_batch_stats(g)) {
        int rows = 0;
        const int rc = launch_bn_stats(x, ldx, n, D, part, st, &rows);
        if (rc) return rc;
        a.part = part, a.nparts = rows;
        a.batch_mean = keep_mean ? keep_mean : b->batch_mean, a.batch_var = keep_var ? keep_var : b->batch_variance;
    }
    a.gamma = b->gamma, a.beta = b->beta, a.moving_mean = b->moving_mean, a.moving_var = b->moving_variance;
    a.eps = g->bn_eps;
    a.one_minus_decay = 1.f - g->bn_decay;
    a.update_moving = g->is_training ? 1 : 0;
    if (g->lns) a.ln_gamma = g->lns[i].gamma, a.ln_beta = g->lns[i].beta;
    const int64_t blocks = (n + kSntRows - 1) / kSntRows;
    hipLaunchKernelGGL(k_snt_norm, dim3((unsigned)blocks), dim3(256), (size_t)2 * D * sizeof(float), st, a);
    GNF_LAUNCH_CHECK("k_snt_norm");
    if (keep_mean && b->batch_mean) {
        const int rc = launch_copy_rows(keep_mean, D, b->batch_mean, D, 1, D, st);
        if (rc) return rc;
    }
    if (keep_var && b->batch_variance) return launch_copy_rows(keep_var, D, b->batch_variance, D, 1, D, st);
    return GNF_OK;
}

EncoderStash encoder_stash(int64_t n, int32_t D, const GnfTimestepGnn* g) {
    EncoderStash s;
    const size_t T = (size_t)g->num_timesteps;
    s.norms = g->bns || g->lns;
    s.buf_floats = ((size_t)n * (size_t)D + 63) / 64 * 64;
    s.dpad = ((size_t)D + 63) / 64 * 64;
    s.v_off = (T - 1) * s.buf_floats;
    s.mom_off = s.v_off + (s.norms ? T * s.buf_floats : 0);
    const size_t floats = s.mom_off + (g->bns ? 2 * T * s.dpad : 0);
    s.total_bytes = (floats ? floats : 64) * sizeof(float);
    return s;
}

// the walk of both forward entry points.  stash == NULL: gnf_timestep_gnn_f32, the rows ping-pong between two workspace
// buffers.  Else the same launches write the rows the backward pass needs straight into their stash regions.
static int run_encoder(const GnfCsr* csr, const GnfTimestepGnn* g, const float* x, int64_t ldx, float* out, int64_t ldo,
                       int32_t D, float* stash, void* ws, hipStream_t st) {
    const int64_t n = csr->n_nodes;
    const EncoderPlan p = encoder_plan(n, D, g);
    const EncoderStash sp = encoder_stash(n, D, g);
    double* part = (double*)ws;
    float* buf[2];
    buf[0] = (float*)((char*)ws + p.part_bytes);
    buf[1] = buf[0] + p.buf_floats;
    float* scratch = buf[1] + p.buf_floats;
    const int T = g->num_timesteps;
    // the rows walk from x through the two buffers to out: every stage writes the buffer its input is not in
    const float* cur = x;
    int64_t ldc = ldx;
    int rc;
    for (int i = 0; i < T; ++i) {
        if (g->bns || g->lns) {
            float* dst = stash ? stash + sp.v_off + (size_t)i * sp.buf_floats : (cur == buf[0] ? buf[1] : buf[0]);
            if (g->bns) {
                float* km = stash ? stash + sp.mom_off + (size_t)(2 * i) * sp.dpad : nullptr;
                rc = launch_snt_norm(g, i, cur, ldc, dst, n, D, part, st, km, km ? km + sp.dpad : nullptr);   // (with this timestep's layer norm, if any)
            } else {
                LnArgs a;
                memset(&a, 0, sizeof(a));
                a.job[0] = LnJob{cur, dst, nullptr, g->lns[i].gamma, g->lns[i].beta};
                a.ldin = ldc, a.ldy = D, a.n = n, a.W = D;
                rc = launch_layer_norm(a, 1, st);
            }
            if (rc) return rc;
            cur = dst, ldc = D;
        }
        const bool last = i == T - 1;
        float* dst = last ? out : (stash ? stash + (size_t)i * sp.buf_floats : (cur == buf[0] ? buf[1] : buf[0]));
        const int64_t ldd = last ? ldo : D;
        rc = launch_gnn_layered(csr->rowptr, csr->col, n, cur, ldc, D, g->gnn, &g->nets[g->weight_sharing ? 0 : i], dst, ldd,
                                scratch, st, csr->node_offsets, csr->n_graphs);
        if (rc) return rc;
        cur = dst, ldc = ldd;
    }
    if (g->residual) return launch_add_rows(out, ldo, x, ldx, n, D, st);
    return GNF_OK;
}

// what both forward entry points check behind validate_encoder
static int check_forward_buffers(const char* what, int64_t n, int32_t D, const GnfTimestepGnn* g, const float* x, int64_t ldx,
                                 const float* out, int64_t ldo, const void* ws, size_t ws_bytes) {
    if (!x || !out || !ws) {
        set_error("%s: null x/out/ws", what);
        return GNF_EINVAL;
    }
    {
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + ((size_t)(n - 1) * (size_t)ldx + (size_t)D) * sizeof(float);
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + ((size_t)(n - 1) * (size_t)ldo + (size_t)D) * sizeof(float);
        if (x0 < o1 && o0 < x1) {
            set_error("%s: x and out overlap (x is never written; the residual reads it last)", what);
            return GNF_EINVAL;
        }
    }
    if ((uintptr_t)ws % sizeof(double)) {
        set_error("%s: ws must be 8-byte aligned (it starts with fp64 moment partials)", what);
        return GNF_EINVAL;
    }
    const EncoderPlan p = encoder_plan(n, D, g);
    if (ws_bytes < p.total_bytes) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, p.total_bytes);
        return GNF_EWORKSPACE;
    }
    return GNF_OK;
}

int validate_encoder_train(const GnfTimestepGnn* g, const char* what) {
    const int n_nets = g->weight_sharing ? 1 : g->num_timesteps;
    for (int q = 0; q < n_nets; ++q)
        if (g->nets[q].attn) {
            set_error("%s: net %d has an attention front-end; the encoder's backward pass covers the message-passing nets only", what, q);
            return GNF_EUNSUPPORTED;
        }
    if (!g->is_training) {
        set_error("%s: needs is_training (the backward pass goes through the batch moments)", what);
        return GNF_EINVAL;
    }
    return GNF_OK;
}

}  // namespace gnf

using namespace gnf;

extern "C" {

size_t gnf_timestep_gnn_workspace_bytes(int64_t n_nodes, int32_t D, const GnfTimestepGnn* g) {
    if (n_nodes < 0 || D < 1 || !g || !g->nets) return 0;
    return encoder_plan(n_nodes, D, g).total_bytes;
}

int gnf_timestep_gnn_f32(const GnfCsr* csr, const GnfTimestepGnn* g, const float* x, int64_t ldx, float* out, int64_t ldo,
                         int32_t D, void* ws, size_t ws_bytes, gnf_stream_t stream) {
    const char* what = "gnf_timestep_gnn_f32";
    int rc = validate_encoder(csr, g, ldx, ldo, D, what);
    if (rc) return rc;
    const int64_t n = csr->n_nodes;
    if (n == 0) return GNF_OK;
    rc = check_forward_buffers(what, n, D, g, x, ldx, out, ldo, ws, ws_bytes);
    if (rc) return rc;
    return run_encoder(csr, g, x, ldx, out, ldo, D, nullptr, ws, (hipStream_t)stream);
}

size_t gnf_timestep_gnn_stash_bytes(int64_t n_nodes, int32_t D, const GnfTimestepGnn* g) {
    if (n_nodes < 0 || n_nodes > kEncMaxNodes || D < 1 || !g || !g->nets || g->num_timesteps < 1) return 0;
    return encoder_stash(n_nodes, D, g).total_bytes;
}

int gnf_timestep_gnn_train_forward_f32(const GnfCsr* csr, const GnfTimestepGnn* g, const float* x, int64_t ldx, float* out,
                                       int64_t ldo, int32_t D, void* stash, size_t stash_bytes, void* ws, size_t ws_bytes,
                                       gnf_stream_t stream) {
    const char* what = "gnf_timestep_gnn_train_forward_f32";
    int rc = validate_encoder(csr, g, ldx, ldo, D, what);
    if (rc) return rc;
    rc = validate_encoder_train(g, what);
    if (rc) return rc;
    const int64_t n = csr->n_nodes;
    if (n == 0) return GNF_OK;
    if (n > kEncMaxNodes) {   // (the backward pass would refuse the stash: refused here already)
        set_error("%s: n_nodes=%lld (at most %lld)", what, (long long)n, (long long)kEncMaxNodes);
        return GNF_EUNSUPPORTED;
    }
    if (!stash || (uintptr_t)stash % sizeof(double)) {
        set_error("%s: null or misaligned stash (8-byte alignment)", what);
        return GNF_EINVAL;
    }
    rc = check_forward_buffers(what, n, D, g, x, ldx, out, ldo, ws, ws_bytes);
    if (rc) return rc;
    const size_t need = encoder_stash(n, D, g).total_bytes;
    if (stash_bytes < need) {
        set_error("%s: stash %zu < %zu bytes", what, stash_bytes, need);
        return GNF_EWORKSPACE;
    }
    return run_encoder(csr, g, x, ldx, out, ldo, D, (float*)stash, ws, (hipStream_t)stream);
}

}  // extern "C"
