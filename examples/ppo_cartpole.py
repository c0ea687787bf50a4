#!/usr/bin/env python
"""PPO on CartPole with every pass over the record inside the library: one launch per epoch.

`rollout_transitions(K, ..., sample=True)` writes whole transitions and `advantages(K, ..., critic=True)` leaves A, R and V per
lane-step, as in `examples/in_kernel_gradients.py`.  One `policy_gradient` call (zero coefficients, its tables are thrown away)
records `old_prob`: its `prob` row is the record's, p[a] under the weights the actions were drawn from.  Then E epochs over the same
record.  Each epoch is one `ppo_gradient` launch -- the ratio p[a] / old_prob, the clip decision and the weight are computed in the
kernel, and the per-policy counters give the clip fraction --, one critic `policy_gradient` launch with the row V - R, and an update
in place in the engine's own tables through `policy_weights_ptr` / `critic_weights_ptr`:

    policy += lr * grad.double() * 2**-24 / (K * n)        (the clipped objective is ascended)

    python examples/ppo_cartpole.py [--lanes 4096] [--steps 64] [--rounds 8] [--epochs 4] [--clip 0.2] [--limit 100] [--hidden 16]
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
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=4, help="E: passes over one record")
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--limit", type=int, default=100, help="max_episode_steps")
    ap.add_argument("--hidden", type=int, default=16, help="H of the critic (0: affine)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n, steps, H, dev = args.lanes, args.steps, args.hidden, "cuda:0"
    gamma, lam, lr_pi, lr_v = 0.97, 0.9, 2.0, 0.05
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
    norm_adv, coef_v, zero, old_prob = f32(steps, stride), f32(steps, stride), f32(steps, stride), f32(steps, stride)
    g_pi, g_v = (torch.zeros((1, t.numel()), dtype=torch.int64, device=dev) for t in (pi_table, v_table))
    x_pi, x_v = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
    counts = torch.zeros((1, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                  lane_stride=stride)

    for r in range(args.rounds):
        env.rollout_transitions(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), sample=True)
        env.advantages(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), advantages=adv.data_ptr(),
                       returns=ret.data_ptr(), values=val.data_ptr(), gamma=gamma, lam=lam, critic=True)  # no sync in between
        # old_prob: the prob row of the weights the record was drawn from (a zero coefficient row: the tables stay zero)
        g_pi.zero_()
        x_pi.zero_()
        torch.cuda.synchronize()
        env.policy_gradient(steps, record=record, start_obs=start.data_ptr(), coef=zero.data_ptr(), grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(),
                            prob=old_prob.data_ptr(), temperature=1.0)
        env.sync()
        A, R = adv[:, :n], ret[:, :n]
        norm_adv[:, :n] = (A - A.mean()) / (A.std() + 1e-6)
        fractions = []
        for _ in range(args.epochs):
            coef_v[:, :n] = val[:, :n] - R  # d/d phi of 0.5 * mean((V - R)^2), V of the record's critic in the first epoch
            for t in (g_pi, g_v, x_pi, x_v, counts):
                t.zero_()  # the launches ADD
            torch.cuda.synchronize()  # torch wrote on its stream; the launches read on the engine's
            env.ppo_gradient(steps, record=record, start_obs=start.data_ptr(), advantages=norm_adv.data_ptr(), old_prob=old_prob.data_ptr(),
                             grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(), counts=counts.data_ptr(), clip=args.clip, temperature=1.0)
            env.policy_gradient(steps, record=record, start_obs=start.data_ptr(), coef=coef_v.data_ptr(), grad=g_v.data_ptr(), excluded=x_v.data_ptr(),
                                critic=True)
            env.sync()
            seen, cut = (int(v) for v in counts[0])
            fractions.append(cut / max(1, seen))
            pi_table += (lr_pi * g_pi[0].double() * 2.0**-24 / (steps * n)).float()  # ascend the clipped objective, in the engine's tables
            v_table -= (lr_v * g_v[0].double() * 2.0**-24 / (steps * n)).float()
            torch.cuda.synchronize()
            # V under the new critic for the next epoch's value row
            env.advantages(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), advantages=coef_v.data_ptr(),
                           values=val.data_ptr(), gamma=gamma, lam=lam, critic=True)
            env.sync()

        ends = int(((done | trunc) != 0)[:, :n].sum())
        env.rollout_closed_loop(steps, fitness=True)  # greedy validation with the new weights
        reward_sum, episodes, _, _ = env.policy_fitness()[0]
        env.policy_fitness_clear()
        print(f"round {r:2d}: {steps * n} sampled transitions, {ends} episode ends, clip fraction per epoch "
              f"{' '.join(f'{f:.3f}' for f in fractions)}, excluded {int(x_pi[0])} + {int(x_v[0])}; greedy validation: "
              f"{int(reward_sum) / max(1, int(episodes) + n):.1f} steps per episode")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
