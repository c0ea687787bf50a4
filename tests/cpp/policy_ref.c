/* policy_ref.c -- the tests' own restatement of the policy of include/gymrs_amd.h ("closed-loop rollouts"), independent of the
 * library: plain C with libm's fmaf (correctly rounded, so the GPU's v_fma_f32 must give the same bits).  Built by
 * tests/test_gpu_policy.py with gcc -O2 -ffp-contract=off.  obs: D rows of n floats (gymrs_obs_ptrs order); act: n bytes. */
#include <math.h>
#include <stdint.h>

void policy_ref(int D, int A, uint32_t H, uint32_t P, uint64_t lanes_per_policy, uint64_t gid0, uint64_t n, const float* weights,
                const float* obs, uint8_t* act)
{
    const uint64_t S = H == 0 ? (uint64_t)A * (D + 1) : (uint64_t)H * (D + 1) + (uint64_t)A * (H + 1);
    for (uint64_t i = 0; i < n; ++i) {
        const float* w = weights + (((gid0 + i) / lanes_per_policy) % P) * S;
        float x[8], y[8];
        for (int j = 0; j < D; ++j) x[j] = obs[(uint64_t)j * n + i];
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
        int action = 0;
        for (int a = 1; a < A; ++a)
            if (y[a] > y[action]) action = a;
        act[i] = (uint8_t)action;
    }
}
