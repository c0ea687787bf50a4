/* policy_ref.c -- the tests' own restatement of the policy of include/gymrs_amd.h ("closed-loop rollouts"), independent of the
 * library: plain C with libm's fmaf (correctly rounded, so the GPU's v_fma_f32 must give the same bits).  Built by
 * tests/closed_loop_ref.py with gcc -O2 -ffp-contract=off.  obs: D rows of n floats (gymrs_obs_ptrs order); act: n bytes. */
#include <math.h>
#include <stdint.h>

/* the logits y[0..A) of one lane under one policy w; z (may be NULL): the H pre-activations of the hidden layer */
static void logits(int D, int A, uint32_t H, const float* w, const float* x, float* y, float* z_out)
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
            if (z_out) z_out[h] = z;
            const float r = (z > 0.0f) ? z : 0.0f;
            for (int a = 0; a < A; ++a) y[a] = fmaf(W2[a * H + h], r, y[a]);
        }
    }
}

static const float* policy_of(int D, int A, uint32_t H, uint32_t P, uint64_t lanes_per_policy, uint64_t g, const float* weights)
{
    const uint64_t S = H == 0 ? (uint64_t)A * (D + 1) : (uint64_t)H * (D + 1) + (uint64_t)A * (H + 1);
    return weights + ((g / lanes_per_policy) % P) * S;
}

void policy_ref(int D, int A, uint32_t H, uint32_t P, uint64_t lanes_per_policy, uint64_t gid0, uint64_t n, const float* weights,
                const float* obs, uint8_t* act)
{
    for (uint64_t i = 0; i < n; ++i) {
        float x[8], y[8];
        for (int j = 0; j < D; ++j) x[j] = obs[(uint64_t)j * n + i];
        logits(D, A, H, policy_of(D, A, H, P, lanes_per_policy, gid0 + i, weights), x, y, 0);
        int action = 0;
        for (int a = 1; a < A; ++a)
            if (y[a] > y[action]) action = a;
        act[i] = (uint8_t)action;
    }
}

/* What policy_ref chose from: y_out A rows of n floats; z_out (may be NULL) H rows of n floats.  For tests that must show that a
 * constructed tie or special value really occurred. */
void policy_ref_logits(int D, int A, uint32_t H, uint32_t P, uint64_t lanes_per_policy, uint64_t gid0, uint64_t n, const float* weights,
                       const float* obs, float* y_out, float* z_out)
{
    for (uint64_t i = 0; i < n; ++i) {
        float x[8], y[8], z[64];
        for (int j = 0; j < D; ++j) x[j] = obs[(uint64_t)j * n + i];
        logits(D, A, H, policy_of(D, A, H, P, lanes_per_policy, gid0 + i, weights), x, y, z);
        for (int a = 0; a < A; ++a) y_out[(uint64_t)a * n + i] = y[a];
        if (z_out)
            for (uint32_t h = 0; h < H; ++h) z_out[(uint64_t)h * n + i] = z[h];
    }
}
