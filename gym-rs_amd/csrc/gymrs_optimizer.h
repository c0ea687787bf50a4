// gymrs_optimizer.h -- the rule of include/gymrs_amd.h, "Optimizer": from one fixed-point table entry to the new weight.  One text for
// the kernel (gymrs_optimizer_impl.h) and for the host (gymrs_optimizer_set): every operation is a single IEEE operation in the order
// written there, fmaf rounds once, divide and square root are the correctly rounded ones (the host's by the language, the device's by
// the compiler's default for HIP, -fhip-fp32-correctly-rounded-divide-sqrt; f32 denormals are kept on gfx950).  Nothing here may be
// contracted or reordered; the library is built with -ffp-contract=off and without fast-math.
//
// What is NOT here is who holds which parameter: the kernel spreads a set over the lanes of a group, the host walks it.
#pragma once
#include "gymrs_math.h"

namespace gymrs {

// g = (float)((double)q * (double)grad_scale): int64 -> f64 to nearest even, one f64 multiply, one rounding to f32
GYMRS_HD float opt_gradient(long long q, float grad_scale) { return (float)((double)q * (double)grad_scale); }

// one term of the norm's sum of squares: exact in f64 (24 x 24 bits)
GYMRS_HD double opt_square(float g) { return (double)g * (double)g; }

// norm = (float)sqrt(slot[0]); the factor of the clip, 1.0f-free: `clipped` says whether g is multiplied at all
GYMRS_HD float opt_clip_scale(double sum, float max_norm, bool& clipped)
{
    const float norm = (float)__builtin_sqrt(sum);
    clipped = norm > max_norm; // (false on NaN)
    return clipped ? max_norm / norm : 1.0f;
}

// The running products of a set, once per call: pw = {p1, p2} advances, c1 and c2 are the bias corrections.
GYMRS_HD void opt_adam_advance(float beta1, float beta2, float& p1, float& p2, float& c1, float& c2)
{
    p1 = p1 * beta1;
    p2 = p2 * beta2;
    c1 = 1.0f - p1;
    c2 = 1.0f - p2;
}

// Adam's step of one parameter; mo and vo are the moments, updated in place.
GYMRS_HD float opt_adam_step(float g, float lr, float beta1, float beta2, float eps, float c1, float c2, float& mo, float& vo)
{
    mo = fmaf_(beta1, mo, (1.0f - beta1) * g);
    vo = fmaf_(beta2, vo, (1.0f - beta2) * (g * g));
    return lr * ((mo / c1) / (__builtin_sqrtf(vo / c2) + eps));
}

GYMRS_HD float opt_sgd_step(float g, float lr) { return lr * g; }

GYMRS_HD float opt_apply(float w, float step, bool ascend) { return ascend ? w + step : w - step; }

// the Polyak average of the target towards the NEW weight
GYMRS_HD float opt_target(float tau, float w_new, float target) { return fmaf_(tau, w_new - target, target); }

} // namespace gymrs
