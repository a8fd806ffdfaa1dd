// The pair logit of the decoders (gnf_decode.hip, gnf_decode_edges.hip) as a kernel argument type: u = logit(d2).
//   DistScaledHacky  what gnf_pred_adj_f32 / gnf_adj_edges_count_f32 launch: one float, the expression they have always had
//   DistSigmoid      include/gnf_distance.h: temp, shift, scale by value and, when `params` is set, temp and shift from device
//                    memory - load() is called once per workgroup, before any pair (an ordinary vector load, see below)
// DistSigmoid spells out what hipcc's contraction makes of temp * (shift - d2 * scale) - one fma, one rounded product - so the
// three files that evaluate it (gnf_adj_loss.hip is the third) cannot drift apart: for (10, 1, 1 / sqrtf(D)) its bits are
// DistScaledHacky's, and tests/test_distance_gpu.py holds them against each other.
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

struct DistScaledHacky {
    float inv_sqrt_d;
    __device__ __forceinline__ DistScaledHacky load() const { return *this; }
    __device__ __forceinline__ float logit(float d2) const { return 10.f * (1.f - d2 * inv_sqrt_d); }
};

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

inline DistSigmoid dist_sigmoid(const GnfDistance& d, int32_t D) {
    DistSigmoid r;
    r.temp = d.temp;
    r.shift = d.shift;
    r.scale = d.scale_by_sqrt_dim ? 1.f / sqrtf((float)D) : 1.f;
    r.params = d.params;
    return r;
}

}  // namespace gnf
