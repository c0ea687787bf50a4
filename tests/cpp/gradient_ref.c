/* gymrs_policy_gradient restated in plain C from the text of include/gymrs_amd.h ("gradients", with the logits of "closed-loop
 * rollouts", the probabilities of "sampling" and the critic of "advantages"): one lane at a time, one parameter array of S floats,
 * no chunks, no vectors.  Built by tests/gradient_ref.py with gcc -O2 -ffp-contract=off; fmaf is libm's (one rounding).  It shares
 * no code with the library. */
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

/* One lane.  w: S floats in the policy layout with A outputs (the critic: A = 1).  x [K][D], act [K] (policy head), coef [K].
 * q [S] is SET, *excluded is SET, prob [K] (may be NULL) is SET. */
void gradient_ref_lane(int D, int A, uint32_t H, int critic, float scale, const float* w, uint32_t K, const float* x, const uint8_t* act,
                       const float* coef, int64_t* q, uint64_t* excluded, float* prob)
{
    const uint32_t S = H == 0 ? (uint32_t)(A * (D + 1)) : H * (uint32_t)(D + 1) + (uint32_t)A * (H + 1);
    const uint32_t o_b1 = H * (uint32_t)D, o_w2 = o_b1 + H, o_b2 = o_w2 + (uint32_t)A * H;
    const float beta = scale * 0x1.62e430p-1f;
    float acc[MAX_S];
    uint32_t k, s, h;
    int b, j;
    for (s = 0; s < S; ++s) acc[s] = 0.0f;
    for (k = 0; k < K; ++k) {
        const float* xk = x + (size_t)k * D;
        const float c = coef[k];
        float g[MAX_A];
        if (critic) {
            g[0] = c;
        } else {
            float y[MAX_A], p[MAX_A];
            const uint8_t a = act[k];
            const float cb = c * beta;
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
            if (prob) prob[k] = a < A ? p[a] : 0.0f;
            if (a >= A) continue; /* contributes nothing */
            for (b = 0; b < A; ++b) g[b] = cb * ((b == a ? 1.0f : 0.0f) - p[b]);
        }
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

/* The whole call: rows as the device has them but n lanes wide (obs [K][D][n], start_obs [D][n], actions / coef / prob [K][n]).
 * grad [n_sets][S] and excluded [n_sets] are ADDED to (modulo 2^64). */
void gradient_ref(int D, int A, uint32_t H, int critic, float scale, uint32_t n_sets, uint64_t lanes_per_set, uint64_t gid0, uint64_t n, uint32_t K,
                  const float* weights, const float* obs, const float* start_obs, const uint8_t* actions, const float* coef, int64_t* grad,
                  uint64_t* excluded, float* prob)
{
    const uint32_t S = H == 0 ? (uint32_t)(A * (D + 1)) : H * (uint32_t)(D + 1) + (uint32_t)A * (H + 1);
    float x[64 * 4], c[64], pr[64];
    uint8_t a[64];
    int64_t q[MAX_S];
    uint64_t i;
    if (K > 64) return;
    for (i = 0; i < n; ++i) {
        const uint32_t set = (uint32_t)(((gid0 + i) / lanes_per_set) % n_sets);
        uint64_t excl = 0;
        uint32_t k, s;
        int j;
        for (k = 0; k < K; ++k) {
            for (j = 0; j < D; ++j) x[k * D + j] = k == 0 ? start_obs[(size_t)j * n + i] : obs[((size_t)(k - 1) * D + j) * n + i];
            c[k] = coef[(size_t)k * n + i];
            a[k] = critic ? 0 : actions[(size_t)k * n + i];
        }
        gradient_ref_lane(D, A, H, critic, scale, weights + (size_t)set * S, K, x, a, c, q, &excl, prob ? pr : 0);
        for (s = 0; s < S; ++s) grad[(size_t)set * S + s] = (int64_t)((uint64_t)grad[(size_t)set * S + s] + (uint64_t)q[s]);
        excluded[set] += excl;
        if (prob)
            for (k = 0; k < K; ++k) prob[(size_t)k * n + i] = pr[k];
    }
}
