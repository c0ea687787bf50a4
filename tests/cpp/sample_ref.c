/* sample_ref.c -- the tests' own restatement of the sampling rule of include/gymrs_amd.h ("sampling"), written from the header's
 * text and independent of the library: plain C with libm's fmaf, floorf and ldexpf (all correctly rounded or exact, so the GPU's
 * instructions must give the same bits).  Built by tests/sample_ref.py with gcc -O2 -ffp-contract=off.  The logits are computed in
 * the order of policy_ref.c.  obs: D rows of n floats (gymrs_obs_ptrs order); words: the Philox word of every lane (drawn by the
 * numpy Philox of tests/explore_ref.py on stream 3). */
#include <math.h>
#include <stdint.h>

static const float C[7] = {1.0f, 0x1.62e430p-1f, 0x1.ebfc40p-3f, 0x1.c69f6ap-5f, 0x1.3c4a8ap-7f, 0x1.4ca4ccp-10f, 0x1.b4d1e4p-13f};

float sample_ref_poly(float f)
{
    float acc = C[6];
    for (int i = 5; i >= 0; --i) acc = fmaf(acc, f, C[i]);
    return acc;
}

float sample_ref_weight(float d)
{
    if (!(d >= -126.0f)) return 0.0f;
    return ldexpf(sample_ref_poly(d - floorf(d)), (int)floorf(d));
}

/* One draw: y[0..A) -> the action; w_out, p_out (may be NULL): the A weights and probabilities.  Returns the greedy action. */
int sample_ref_draw(int A, const float* y, float scale, uint32_t word, uint8_t* action, float* w_out, float* p_out)
{
    float w[8];
    int greedy = 0;
    for (int a = 1; a < A; ++a)
        if (y[a] > y[greedy]) greedy = a;
    const float m = y[greedy];
    for (int a = 0; a < A; ++a) {
        const float diff = y[a] - m;
        const float d = diff * scale;
        w[a] = sample_ref_weight(d);
    }
    float total = w[0] + w[1];
    for (int a = 2; a < A; ++a) total = total + w[a];
    const float u = (float)(word >> 8) * 0x1p-24f;
    const float thr = u * total;
    int chosen = -1;
    float run = 0.0f;
    for (int a = 0; a < A && chosen < 0; ++a) {
        run = (a == 0) ? w[0] : run + w[a];
        if (thr < run) chosen = a;
    }
    if (chosen < 0) chosen = greedy;
    *action = (uint8_t)chosen;
    for (int a = 0; a < A; ++a) {
        if (w_out) w_out[a] = w[a];
        if (p_out) p_out[a] = (total > 0.0f) ? w[a] / total : (a == greedy ? 1.0f : 0.0f);
    }
    return greedy;
}

/* n draws from one row of logits each: y is [n][A], words [n]; act [n], greedy [n], probs [n][A] (may be NULL) */
void sample_ref_draw_many(int A, uint64_t n, const float* y, float scale, const uint32_t* words, uint8_t* act, uint8_t* greedy, float* probs)
{
    for (uint64_t i = 0; i < n; ++i) greedy[i] = (uint8_t)sample_ref_draw(A, y + i * A, scale, words[i], act + i, 0, probs ? probs + i * A : 0);
}

/* policy_ref.c's logits, restated */
static void logits(int D, int A, uint32_t H, const float* w, const float* x, float* y)
{
    if (H == 0) {
        const float *W = w, *b = w + A * D;
        for (int a = 0; a < A; ++a) {
            y[a] = b[a];
            for (int j = 0; j < D; ++j) y[a] = fmaf(W[a * D + j], x[j], y[a]);
        }
    } else {
        const float *W1 = w, *b1 = W1 + H * D, *W2 = b1 + H, *b2 = W2 + A * H;
        for (int a = 0; a < A; ++a) y[a] = b2[a];
        for (uint32_t h = 0; h < H; ++h) {
            float z = b1[h];
            for (int j = 0; j < D; ++j) z = fmaf(W1[h * D + j], x[j], z);
            const float r = (z > 0.0f) ? z : 0.0f;
            for (int a = 0; a < A; ++a) y[a] = fmaf(W2[a * H + h], r, y[a]);
        }
    }
}

/* The sampled actions of n lanes (lane i is global id gid0 + i): act, greedy, prob (of the action taken) [n]; y_out (may be NULL) [A][n] */
void sample_ref(int D, int A, uint32_t H, uint32_t P, uint64_t lanes_per_policy, uint64_t gid0, uint64_t n, const float* weights, const float* obs,
                float scale, const uint32_t* words, uint8_t* act, uint8_t* greedy, float* prob, float* y_out)
{
    const uint64_t S = H == 0 ? (uint64_t)A * (D + 1) : (uint64_t)H * (D + 1) + (uint64_t)A * (H + 1);
    for (uint64_t i = 0; i < n; ++i) {
        float x[8], y[8], p[8];
        for (int j = 0; j < D; ++j) x[j] = obs[(uint64_t)j * n + i];
        logits(D, A, H, weights + (((gid0 + i) / lanes_per_policy) % P) * S, x, y);
        greedy[i] = (uint8_t)sample_ref_draw(A, y, scale, words[i], act + i, 0, p);
        prob[i] = p[act[i]];
        if (y_out)
            for (int a = 0; a < A; ++a) y_out[(uint64_t)a * n + i] = y[a];
    }
}

/* max over f = i / 2^23, i in [0, 2^23), of |P(f) - 2^f| / 2^f, P with true fmaf, the rest in f64 */
double sample_ref_poly_max_rel_err(void)
{
    double worst = 0.0;
    for (uint32_t i = 0; i < (1u << 23); ++i) {
        const float f = (float)i * 0x1p-23f;
        const double want = exp2((double)f);
        const double err = fabs((double)sample_ref_poly(f) - want) / want;
        if (err > worst) worst = err;
    }
    return worst;
}
