// What the files that score embeddings pair by pair inside each graph share (gnf_decode.hip, gnf_decode_edges.hip,
// gnf_adj_loss.hip): the pair logit u = logit(d2) as ONE kernel argument type, the staging of a tile's rows in LDS, the
// fmaf chain of d2 and the scan that turns n_node into node offsets (declared here, defined in gnf_decode.hip).
//   DistSigmoid   include/gnf_distance.h: temp, shift, scale by value and, when `params` is set, temp and shift from device
//                 memory - load() is called once per workgroup, before any pair (an ordinary vector load, see below)
// The logit is spelled out - one fma, one rounded product - so no compiler flag decides its bits; the entry points without a
// GnfDistance argument pass dist_scaled_hacky(D), the function they have always computed.
#pragma once
#include "gnf_common.h"

namespace gnf {

// temp and shift in device memory are rewritten by another kernel (the optimiser's step) between two launches: they are read
// with an ordinary vector load that is coherent at device scope (a plain load of a uniform address would go through the scalar
// cache).  tests/test_distance_gpu.py records what a replayed capture does with them.
__device__ __forceinline__ float load_dist_param(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ float sigmoid_l2_logit(float temp, float shift, float scale, float d2) {
    return __fmul_rn(temp, fmaf(-d2, scale, shift));
}

struct DistSigmoid {
    float temp, shift, scale;
    const float* params;   // NULL, or device {temp, shift}
    __device__ __forceinline__ DistSigmoid load() const {
        DistSigmoid r = *this;
        if (params) {
            r.temp = load_dist_param(params);
            r.shift = load_dist_param(params + 1);
        }
        return r;
    }
    __device__ __forceinline__ float logit(float d2) const { return sigmoid_l2_logit(temp, shift, scale, d2); }
};

inline DistSigmoid dist_sigmoid(float temp, float shift, int32_t scale_by_sqrt_dim, const float* params, int32_t D) {
    return DistSigmoid{temp, shift, scale_by_sqrt_dim ? 1.f / sqrtf((float)(D >= 1 ? D : 1)) : 1.f, params};
}
inline DistSigmoid dist_sigmoid(const GnfDistance& d, int32_t D) {
    return dist_sigmoid(d.temp, d.shift, d.scale_by_sqrt_dim, d.params, D);
}
// scaled_hacky_sigmoid_l2 (loss.py:45-53): sigmoid(10 (1 - d2 / sqrt(D)))
inline DistSigmoid dist_scaled_hacky(int32_t D) { return dist_sigmoid(10.f, 1.f, 1, nullptr, D); }

// rows [row0, row0 + rows) of z -> tile [rows][D] in LDS, by the 256 lanes of a workgroup; the caller synchronises
__device__ __forceinline__ void stage_row_tile(float* tile, const float* __restrict__ z, int64_t ld, int D, int64_t row0,
                                               int rows) {
    for (int i = threadIdx.x; i < rows * D; i += 256) {
        const int rl = i / D, f = i - rl * D;
        tile[i] = z[(row0 + rl) * ld + f];
    }
}

// d2[q] = ||zr[q] - zc||^2, q < R: one fmaf chain per row over the features in ascending order, zc[f] read once for all rows.
// Every kernel of the three files forms d2 here, so a pair has the same d2 bits in all of them.
template <int R>
__device__ __forceinline__ void pair_d2(const float* const (&zr)[R], const float* zc, int D, float (&d2)[R]) {
#pragma unroll
    for (int q = 0; q < R; ++q) d2[q] = 0.f;
    for (int f = 0; f < D; ++f) {
        const float zcf = zc[f];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const float df = zr[q][f] - zcf;
            d2[q] = fmaf(df, df, d2[q]);
        }
    }
}

// node_off[g] = n_node[0] + ... + n_node[g - 1], g <= n_graphs, on the stream (k_node_offsets, gnf_decode.hip: one workgroup,
// any n_graphs); blk_off, when not NULL, gets the same over n_node^2 - the offsets of the [n_g, n_g] blocks.
int launch_node_offsets(const int32_t* n_node, int64_t n_graphs, int64_t* node_off, int64_t* blk_off, hipStream_t st);

}  // namespace gnf
