/* gymrs_ppo_gradient restated in plain C from the text of include/gymrs_amd.h ("clipped surrogate", with the backward pass and the
 * fixed point of "gradients", the logits of "closed-loop rollouts" and the probabilities of "sampling"): one lane at a time, one
 * parameter array of S floats, no chunks, no vectors.  Built by tests/ppo_ref.py with gcc -O2 -ffp-contract=off; fmaf is libm's (one
 * rounding).  It shares no code with the library and none with tests/cpp/gradient_ref.c. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAX_A 3
#define MAX_S 512

static float exp2_poly(float f)
{
    float acc = 0x1.b4d1e4p-13f;
    acc = fmaf(acc, f, 0x1.4ca4ccp-10f);
    acc = fmaf(acc, f, 0x1.3c4a8ap-7f);
    acc = fmaf(acc, f, 0x1.c69f6ap-5f);
    acc = fmaf(acc, f, 0x1.ebfc40p-3f);
    acc = fmaf(acc, f, 0x1.62e430p-1f);
    acc = fmaf(acc, f, 1.0f);
    return acc;
}

static float weight_of(float d)
{
    float fl;
    if (!(d >= -126.0f)) return 0.0f;
    fl = floorf(d);
    return ldexpf(exp2_poly(d - fl), (int)fl);
}

/* p[0..A) of the sampling rule for the logits y */
static void probabilities(const float* y, int A, float scale, float* p)
{
    int greedy = 0, a;
    float w[MAX_A], total;
    for (a = 1; a < A; ++a)
        if (y[a] > y[greedy]) greedy = a;
    for (a = 0; a < A; ++a) w[a] = weight_of((y[a] - y[greedy]) * scale);
    total = w[0];
    for (a = 1; a < A; ++a) total = total + w[a];
    for (a = 0; a < A; ++a) p[a] = (total > 0.0f) ? w[a] / total : (a == greedy ? 1.0f : 0.0f);
}

/* One lane.  w: S floats in the policy layout.  x [K][D], act [K], adv [K], old_prob [K].  q [S], *excluded and counts [2] are SET,
 * prob [K] and coef [K] (the c of every step, +0 where a >= A; either may be NULL) are SET. */
void ppo_ref_lane(int D, int A, uint32_t H, float scale, float clip_low, float clip_high, const float* w, uint32_t K, const float* x,
                  const uint8_t* act, const float* adv, const float* old_prob, int64_t* q, uint64_t* excluded, uint64_t* counts, float* prob,
                  float* coef)
{
    const uint32_t S = H == 0 ? (uint32_t)(A * (D + 1)) : H * (uint32_t)(D + 1) + (uint32_t)A * (H + 1);
    const uint32_t o_b1 = H * (uint32_t)D, o_w2 = o_b1 + H, o_b2 = o_w2 + (uint32_t)A * H;
    const float beta = scale * 0x1.62e430p-1f;
    float acc[MAX_S];
    uint32_t k, s, h;
    int b, j;
    for (s = 0; s < S; ++s) acc[s] = 0.0f;
    counts[0] = counts[1] = 0;
    for (k = 0; k < K; ++k) {
        const float* xk = x + (size_t)k * D;
        float g[MAX_A], y[MAX_A], p[MAX_A], pa, ratio, c, cb;
        const uint8_t a = act[k];
        int cut;
        if (H == 0) {
            for (b = 0; b < A; ++b) {
                y[b] = w[A * D + b];
                for (j = 0; j < D; ++j) y[b] = fmaf(w[b * D + j], xk[j], y[b]);
            }
        } else {
            for (b = 0; b < A; ++b) y[b] = w[o_b2 + b];
            for (h = 0; h < H; ++h) {
                float z = w[o_b1 + h], r;
                for (j = 0; j < D; ++j) z = fmaf(w[h * D + j], xk[j], z);
                r = (z > 0.0f) ? z : 0.0f;
                for (b = 0; b < A; ++b) y[b] = fmaf(w[o_w2 + b * H + h], r, y[b]);
            }
        }
        probabilities(y, A, scale, p);
        pa = a < A ? p[a] : 0.0f;
        if (prob) prob[k] = pa;
        if (coef) coef[k] = 0.0f;
        if (a >= A) continue; /* contributes nothing, is not counted */
        ratio = pa / old_prob[k];
        cut = (adv[k] > 0.0f && ratio > clip_high) || (adv[k] < 0.0f && ratio < clip_low);
        c = cut ? 0.0f : adv[k] * ratio;
        if (coef) coef[k] = c;
        counts[0] += 1;
        counts[1] += cut ? 1 : 0;
        cb = c * beta;
        for (b = 0; b < A; ++b) g[b] = cb * ((b == a ? 1.0f : 0.0f) - p[b]);
        if (H == 0) {
            for (b = 0; b < A; ++b) {
                for (j = 0; j < D; ++j) acc[b * D + j] = fmaf(g[b], xk[j], acc[b * D + j]);
                acc[A * D + b] = acc[A * D + b] + g[b];
            }
        } else {
            for (b = 0; b < A; ++b) acc[o_b2 + b] = acc[o_b2 + b] + g[b];
            for (h = 0; h < H; ++h) {
                float z = w[o_b1 + h], r, e, dz;
                for (j = 0; j < D; ++j) z = fmaf(w[h * D + j], xk[j], z);
                r = (z > 0.0f) ? z : 0.0f;
                for (b = 0; b < A; ++b) acc[o_w2 + b * H + h] = fmaf(g[b], r, acc[o_w2 + b * H + h]);
                e = g[0] * w[o_w2 + h];
                for (b = 1; b < A; ++b) e = fmaf(g[b], w[o_w2 + b * H + h], e);
                dz = (z > 0.0f) ? e : 0.0f;
                acc[o_b1 + h] = acc[o_b1 + h] + dz;
                for (j = 0; j < D; ++j) acc[h * D + j] = fmaf(dz, xk[j], acc[h * D + j]);
            }
        }
    }
    *excluded = 0;
    for (s = 0; s < S; ++s) {
        const float L = acc[s];
        if (isfinite(L) && fabsf(L) < 0x1p30f) {
            q[s] = (int64_t)rint((double)L * 16777216.0);
        } else {
            q[s] = 0;
            *excluded += 1;
        }
    }
}

/* The whole call: rows as the device has them but n lanes wide (obs [K][D][n], start_obs [D][n], actions / advantages / old_prob / prob
 * / coef [K][n]).  grad [n_sets][S], excluded [n_sets] and counts [n_sets][2] are ADDED to (modulo 2^64); prob and coef (either may be
 * NULL) are SET. */
void ppo_ref(int D, int A, uint32_t H, float scale, float clip_low, float clip_high, uint32_t n_sets, uint64_t lanes_per_set, uint64_t gid0, uint64_t n,
             uint32_t K, const float* weights, const float* obs, const float* start_obs, const uint8_t* actions, const float* advantages,
             const float* old_prob, int64_t* grad, uint64_t* excluded, uint64_t* counts, float* prob, float* coef)
{
    const uint32_t S = H == 0 ? (uint32_t)(A * (D + 1)) : H * (uint32_t)(D + 1) + (uint32_t)A * (H + 1);
    float x[64 * 4], ad[64], po[64], pr[64], cf[64];
    uint8_t a[64];
    int64_t q[MAX_S];
    uint64_t i;
    if (K > 64) return;
    for (i = 0; i < n; ++i) {
        const uint32_t set = (uint32_t)(((gid0 + i) / lanes_per_set) % n_sets);
        uint64_t excl = 0, cnt[2];
        uint32_t k, s;
        int j;
        for (k = 0; k < K; ++k) {
            for (j = 0; j < D; ++j) x[k * D + j] = k == 0 ? start_obs[(size_t)j * n + i] : obs[((size_t)(k - 1) * D + j) * n + i];
            ad[k] = advantages[(size_t)k * n + i];
            po[k] = old_prob[(size_t)k * n + i];
            a[k] = actions[(size_t)k * n + i];
        }
        ppo_ref_lane(D, A, H, scale, clip_low, clip_high, weights + (size_t)set * S, K, x, a, ad, po, q, &excl, cnt, pr, cf);
        for (s = 0; s < S; ++s) grad[(size_t)set * S + s] = (int64_t)((uint64_t)grad[(size_t)set * S + s] + (uint64_t)q[s]);
        excluded[set] += excl;
        counts[(size_t)set * 2] += cnt[0];
        counts[(size_t)set * 2 + 1] += cnt[1];
        for (k = 0; k < K; ++k) {
            if (prob) prob[(size_t)k * n + i] = pr[k];
            if (coef) coef[(size_t)k * n + i] = cf[k];
        }
    }
}
