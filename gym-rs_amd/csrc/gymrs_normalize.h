// gymrs_normalize.h -- the rule of include/gymrs_amd.h, "advantage normalisation": per-set standardisation of an advantages row
// through integer sums.  One text for the kernels (gymrs_normalize_impl.h) and for the host (gymrs_normalize_host).  A member's
// share of every sum is an integer before members are added, and the sums are integers modulo 2^64: within one engine the statistics
// do not depend on scheduling or tiling.  Over engines that cut one batch only S1, n and non_members add up: S2 is centred on the
// mean of the engine's own members, so S2, mean, inv and out are per engine.  Resolution: 2^-24 on an element (first sum) and on a square (second
// sum).  No wrap while, per set, |sum of A| < 2^39 and the sum of (A - mean)^2 < 2^40.  The f64 operations (divide, sqrt, the
// conversions) are single correctly rounded IEEE operations on the host and on gfx950 alike.
#pragma once
#include "gymrs_math.h"

namespace gymrs {

// A is finite and |A| < 8192: it enters the statistics.  Everything else (NaN, the infinities, an outlier) is written but not counted.
GYMRS_HD bool normalize_member(float A) { return fabsf_(A) < 8192.0f; }

// pass 1: |q1| < 2^37, exact in f64 before the rounding
GYMRS_HD long long normalize_q1(float A) { return (long long)__builtin_rint((double)A * 16777216.0); }

GYMRS_HD float normalize_mean(long long s1, unsigned long long n)
{
    return n == 0 ? 0.0f : (float)((double)s1 / ((double)n * 16777216.0));
}

// pass 2: |A - mean| < 16384, so sq < 2^28 and q2 < 2^52: it always fixes
GYMRS_HD unsigned long long normalize_q2(float A, float mean)
{
    const float dm = A - mean;
    const float sq = dm * dm;
    return (unsigned long long)__builtin_rint((double)sq * 16777216.0);
}

// 1 / (sd + eps), sd = the sample standard deviation (n - 1); n < 2: sd = 0
GYMRS_HD float normalize_inv(unsigned long long s2, unsigned long long n, float eps)
{
    const double var = n < 2 ? 0.0 : (double)s2 / 16777216.0 / (double)(n - 1);
    const double sd = __builtin_sqrt(var);
    return (float)(1.0 / (sd + (double)eps));
}

// pass 3, for EVERY element: a non-member gets the same arithmetic (NaN stays NaN)
GYMRS_HD float normalize_out(float A, float mean, float inv) { return (A - mean) * inv; }

} // namespace gymrs
