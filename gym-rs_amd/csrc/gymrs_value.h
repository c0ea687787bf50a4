// gymrs_value.h -- the rule of include/gymrs_amd.h, "value loss": the coefficient of the critic head computed from the critic's own
// forward pass, a returns row and (GYMRS_VALUE_CLIP) an old-values row.  One text for the kernels (gymrs_value_impl.h) and for the
// host (gymrs_value_lane): every operation is a single IEEE f32 operation in the order written here, every `?:` a select.  Nothing
// here may be contracted or reordered; the library is built with -ffp-contract=off and without fast-math.
#pragma once
#include "gymrs_advantages.h"
#include "gymrs_gradient.h"

namespace gymrs {

// c of one lane-step.  clipped: GYMRS_VALUE_CLIP (vo and clip are read).  e1 = v - R; es = the error whose square is the larger one
// (e2 where cut, else e1); cut = the clipped value is in use and its error is the larger one: the lane-step adds nothing.
// The compares are false on NaN: a NaN vo is neither above nor below the range, so v is used as it is.
GYMRS_HD float value_coefficient(float v, float R, float vo, float clip, bool clipped, float& e1, float& es, bool& cut)
{
    e1 = v - R;
    const float dl = v - vo;
    const bool hi = clipped && dl > clip, lo = clipped && dl < -clip;
    const float vc = hi ? vo + clip : (lo ? vo - clip : v);
    const float e2 = vc - R;
    cut = (hi || lo) && (e2 * e2 > e1 * e1);
    es = cut ? e2 : e1;
    return cut ? 0.0f : e1;
}

// The two running sums and the counters of a lane, in step order: s0 += e1^2, s1 += es^2 (one fused multiply-add each).
template <int VEC>
struct ValueSums {
    float s0[VEC], s1[VEC];
    uint32_t seen[VEC], cut[VEC];
};

// One lane-step of every lane of a caller: g = c, and (SUMS) the lane's sums and counters.
template <int VEC, bool SUMS>
GYMRS_HD void value_head(const float (&v)[VEC], const float (&R)[VEC], const float (&vo)[VEC], float clip, bool clipped, float (&g)[1][VEC],
                         ValueSums<VEC>& sums)
{
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        float e1, es;
        bool cut;
        g[0][k] = value_coefficient(v[k], R[k], vo[k], clip, clipped, e1, es, cut);
        if constexpr (SUMS) {
            sums.s0[k] = fmaf_(e1, e1, sums.s0[k]);
            sums.s1[k] = fmaf_(es, es, sums.s1[k]);
            sums.seen[k] += 1u;
            sums.cut[k] += cut ? 1u : 0u;
        }
    }
}

} // namespace gymrs
