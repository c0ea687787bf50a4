/* The rule of include/gymrs_amd.h, "advantages", restated in plain C from the header's text: the critic (the policy network with one
 * output) and the GAE(lambda) backward scan over a transitions record.  libm's fmaf, gcc -O2 -ffp-contract=off: every operation is
 * the single IEEE f32 operation the header names, every `?:` a select.  Shares no code with the library. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* V(x) under one critic w: H == 0: W[D], b; H > 0: W1[H][D], b1[H], W2[H], b2 */
float advantages_ref_critic(int d, uint32_t hidden, const float* w, const float* x)
{
    if (hidden == 0) {
        float v = w[d];
        for (int j = 0; j < d; ++j) v = fmaf(w[j], x[j], v);
        return v;
    }
    const float* w1 = w;
    const float* b1 = w1 + (size_t)hidden * d;
    const float* w2 = b1 + hidden;
    float v = w2[hidden];
    for (uint32_t h = 0; h < hidden; ++h) {
        float z = b1[h];
        for (int j = 0; j < d; ++j) z = fmaf(w1[(size_t)h * d + j], x[j], z);
        const float r = (z > 0.0f) ? z : 0.0f;
        v = fmaf(w2[h], r, v);
    }
    return v;
}

static size_t critic_size(int d, uint32_t hidden) { return hidden == 0 ? (size_t)d + 1 : (size_t)hidden * (d + 2) + 1; }

/* V of column i of x [d][n] (lane gid0 + i of the batch); w == NULL: +0.0f */
static float value_of(int d, uint32_t hidden, uint32_t n_critics, uint64_t lanes_per_critic, uint64_t gid0, const float* w, const float* x, uint64_t n,
                      uint64_t i)
{
    float col[4];
    if (!w) return 0.0f;
    for (int j = 0; j < d; ++j) col[j] = x[(size_t)j * n + i];
    const uint64_t c = ((gid0 + i) / lanes_per_critic) % n_critics;
    return advantages_ref_critic(d, hidden, w + c * critic_size(d, hidden), col);
}

/* values of the columns of x [d][n] */
void advantages_ref_values(int d, uint32_t hidden, uint32_t n_critics, uint64_t lanes_per_critic, uint64_t gid0, uint64_t n, const float* w, const float* x,
                           float* v)
{
    for (uint64_t i = 0; i < n; ++i) v[i] = value_of(d, hidden, n_critics, lanes_per_critic, gid0, w, x, n, i);
}

/* The scan.  obs, final_obs [K][d][n], start_obs [d][n], reward, done, truncated, adv, ret, val [K][n]; w == NULL: no critic;
 * truncated, final_obs may be NULL. */
void advantages_ref(int d, uint32_t hidden, uint32_t n_critics, uint64_t lanes_per_critic, uint64_t gid0, uint64_t n, uint32_t n_steps, const float* w,
                    const float* obs, const float* reward, const uint8_t* done, const uint8_t* truncated, const float* final_obs, const float* start_obs,
                    float gamma, float lambda, float* adv, float* ret, float* val)
{
    const float gl = gamma * lambda;
    const size_t row = (size_t)d * n;
    for (uint64_t i = 0; i < n; ++i) {
        float next = 0.0f; /* A[k + 1] */
        for (uint32_t k = n_steps; k-- > 0;) {
            const size_t at = (size_t)k * n + i;
            const int ended = done[at] != 0 || (truncated != NULL && truncated[at] != 0);
            const float* x_next = (final_obs != NULL && ended) ? final_obs + k * row : obs + k * row;
            const float v_next = done[at] != 0 ? 0.0f : value_of(d, hidden, n_critics, lanes_per_critic, gid0, w, x_next, n, i);
            const float v_cur = value_of(d, hidden, n_critics, lanes_per_critic, gid0, w, k == 0 ? start_obs : obs + (k - 1) * row, n, i);
            const float delta = fmaf(gamma, v_next, reward[at]) - v_cur;
            const float carry = ended ? 0.0f : next;
            const float a = fmaf(gl, carry, delta);
            adv[at] = a;
            ret[at] = a + v_cur;
            val[at] = v_cur;
            next = a;
        }
    }
}
