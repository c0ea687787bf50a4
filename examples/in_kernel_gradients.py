#!/usr/bin/env python
"""Actor-critic on CartPole with every stage inside the library: collect, targets, gradients.

The loop of `examples/actor_critic_collection.py` with both torch autograd steps replaced by two `policy_gradient` launches.
`rollout_transitions(K, ..., sample=True)` writes whole transitions, `advantages(K, ..., critic=True)` leaves A, R and V per
lane-step, torch fills two coefficient rows with element-wise operations (`-(A - mean) / std` for the policy, `V - R` for the critic)
and `policy_gradient` turns each into its exact fixed-point gradient table in one pass over the record: no `[K, A, n]` or
`[K, H, n]` intermediate exists.  The update is in place in the engine's own tables:

    table -= lr * grad.double() * 2**-24 / (K * n)

In the first round the autograd gradient of the other example's losses is computed once beside it and the largest difference printed.

    python examples/in_kernel_gradients.py [--lanes 4096] [--steps 64] [--rounds 12] [--limit 100] [--hidden 16]
"""
from __future__ import annotations

import argparse
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
gymrs = importlib.import_module("gym-rs_amd")


class DeviceFloats:
    """n floats at a device address, for torch.as_tensor (zero-copy)"""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64, help="K: steps per launch")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--limit", type=int, default=100, help="max_episode_steps")
    ap.add_argument("--hidden", type=int, default=16, help="H of the critic (0: affine)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n, steps, H, dev = args.lanes, args.steps, args.hidden, "cuda:0"
    gamma, lam, lr_pi, lr_v = 0.97, 0.9, 0.5, 0.05
    rng = np.random.default_rng(args.seed)
    policy = (0.1 * rng.standard_normal(gymrs.policy_size(gymrs.CARTPOLE, 0))).astype(np.float32)  # W[2][4], b[2]
    critic = (0.1 * rng.standard_normal(gymrs.critic_size(gymrs.CARTPOLE, H))).astype(np.float32)  # W1[H][4], b1[H], W2[H], b2

    params = gymrs.engine.default_params(gymrs.CARTPOLE)
    params.max_episode_steps = args.limit
    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT, params=params)
    env.reset(seed=args.seed)
    env.set_policy(policy, hidden=0, lanes_per_policy=n)
    env.set_critic(critic, hidden=H, lanes_per_critic=n)
    env.set_sampling(4321, temperature=1.0)
    pi_table = torch.as_tensor(DeviceFloats(*env.policy_weights_ptr()), device=dev)  # the engine's own weights
    v_table = torch.as_tensor(DeviceFloats(*env.critic_weights_ptr()), device=dev)

    stride = (n + 15) // 16 * 16
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    obs, final, start, rew = f32(steps, 4, stride), f32(steps, 4, stride), f32(4, stride), f32(steps, stride)
    act, done, trunc = u8(steps, stride), u8(steps, stride), u8(steps, stride)
    adv, ret, val = f32(steps, stride), f32(steps, stride), f32(steps, stride)
    coef_pi, coef_v = f32(steps, stride), f32(steps, stride)
    g_pi, g_v = (torch.zeros((1, t.numel()), dtype=torch.int64, device=dev) for t in (pi_table, v_table))
    x_pi, x_v = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                  lane_stride=stride)

    def autograd_gradients():  # the update of examples/actor_critic_collection.py, for the comparison of the first round
        s = torch.cat([start[None, :, :n], obs[:-1, :, :n]])
        A, R = adv[:, :n], ret[:, :n]
        theta = pi_table.clone().requires_grad_(True)
        logits = torch.einsum("aj,kjn->kan", theta[:8].reshape(2, 4), s) + theta[8:][None, :, None]
        logp = torch.log_softmax(logits, dim=1).gather(1, act[:, :n].long()[:, None, :]).squeeze(1)
        (-(logp * (A - A.mean()) / (A.std() + 1e-6)).mean()).backward()
        phi = v_table.clone().requires_grad_(True)
        if H == 0:
            v = torch.einsum("j,kjn->kn", phi[:4], s) + phi[4]
        else:
            w1, b1, w2, b2 = phi[:4 * H].reshape(H, 4), phi[4 * H:5 * H], phi[5 * H:6 * H], phi[6 * H]
            v = torch.einsum("h,khn->kn", w2, torch.relu(torch.einsum("hj,kjn->khn", w1, s) + b1[None, :, None])) + b2
        (0.5 * ((v - R) ** 2).mean()).backward()
        return theta.grad, phi.grad

    for r in range(args.rounds):
        env.rollout_transitions(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), sample=True)
        env.advantages(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), advantages=adv.data_ptr(),
                       returns=ret.data_ptr(), values=val.data_ptr(), gamma=gamma, lam=lam, critic=True)  # no sync in between
        env.sync()

        # the coefficient rows: element-wise torch on [K, n], nothing larger
        A, R, V = adv[:, :n], ret[:, :n], val[:, :n]
        coef_pi[:, :n] = -(A - A.mean()) / (A.std() + 1e-6)  # d/d theta of -mean(log pi * normalised A)
        coef_v[:, :n] = V - R                                # d/d phi of 0.5 * mean((V - R)^2)
        for t in (g_pi, g_v, x_pi, x_v):
            t.zero_()  # the launches ADD
        torch.cuda.synchronize()  # torch wrote on its stream; the launches read on the engine's
        env.policy_gradient(steps, record=record, start_obs=start.data_ptr(), coef=coef_pi.data_ptr(), grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(),
                            temperature=1.0)
        env.policy_gradient(steps, record=record, start_obs=start.data_ptr(), coef=coef_v.data_ptr(), grad=g_v.data_ptr(), excluded=x_v.data_ptr(),
                            critic=True)
        env.sync()
        d_pi = g_pi[0].double() * 2.0**-24 / (steps * n)
        d_v = g_v[0].double() * 2.0**-24 / (steps * n)
        if r == 0:
            t_pi, t_v = autograd_gradients()
            print(f"largest difference to the autograd gradient: policy {(d_pi - t_pi.double()).abs().max().item():.3e} (largest entry "
                  f"{t_pi.abs().max().item():.3e}), critic {(d_v - t_v.double()).abs().max().item():.3e} (largest entry {t_v.abs().max().item():.3e})")
        pi_table -= (lr_pi * d_pi).float()  # in place, in the engine's tables
        v_table -= (lr_v * d_v).float()
        torch.cuda.synchronize()

        ends = int(((done | trunc) != 0)[:, :n].sum())
        env.rollout_closed_loop(steps, fitness=True)  # greedy validation with the new weights
        reward_sum, episodes, _, _ = env.policy_fitness()[0]
        env.policy_fitness_clear()
        print(f"round {r:2d}: {steps * n} sampled transitions, {ends} episode ends, mean V {V.mean().item():.3f}, mean R {R.mean().item():.3f}, "
              f"excluded {int(x_pi[0])} + {int(x_v[0])}; greedy validation: {int(reward_sum) / max(1, int(episodes) + n):.1f} steps per episode")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
