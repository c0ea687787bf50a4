#!/usr/bin/env python
"""Actor-critic collection from two launches: sampled transitions, then GAE(lambda) advantages and returns, on CartPole.

`rollout_transitions(K, ..., sample=True)` plays a ~ softmax(logits) inside the kernel and writes whole transitions;
`advantages(K, ..., critic=True)`, enqueued right behind it on the engine's stream, evaluates the critic inside its kernel and leaves
the learner's targets: A (advantages) and R (returns) per lane-step, truncated steps bootstrapped from `final_obs`, done steps not.
torch then takes one gradient step on the policy (the policy-gradient loss with A) and one on the critic (the squared error to R),
both written straight into the engine's tables through `policy_weights_ptr` and `critic_weights_ptr` (zero-copy), so the next round
plays and evaluates the new weights without a `set_policy` / `set_critic`.

    python examples/actor_critic_collection.py [--lanes 4096] [--steps 64] [--rounds 12] [--limit 100] [--hidden 16]
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
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                  lane_stride=stride)

    def value(theta, s):  # the critic in torch, for the gradient: the layout of include/gymrs_amd.h, "advantages"
        if H == 0:
            return torch.einsum("j,kjn->kn", theta[:4], s) + theta[4]
        w1, b1, w2, b2 = theta[:4 * H].reshape(H, 4), theta[4 * H:5 * H], theta[5 * H:6 * H], theta[6 * H]
        return torch.einsum("h,khn->kn", w2, torch.relu(torch.einsum("hj,kjn->khn", w1, s) + b1[None, :, None])) + b2

    for r in range(args.rounds):
        env.rollout_transitions(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), sample=True)
        env.advantages(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), advantages=adv.data_ptr(),
                       returns=ret.data_ptr(), values=val.data_ptr(), gamma=gamma, lam=lam, critic=True)  # no sync in between
        env.sync()

        # the (s, a, A, R) rows: s is the observation the action was drawn from
        s = torch.cat([start[None, :, :n], obs[:-1, :, :n]])
        a = act[:, :n].long()
        A, R = adv[:, :n], ret[:, :n]
        theta = pi_table.clone().requires_grad_(True)
        logits = torch.einsum("aj,kjn->kan", theta[:8].reshape(2, 4), s) + theta[8:][None, :, None]
        logp = torch.log_softmax(logits, dim=1).gather(1, a[:, None, :]).squeeze(1)
        pi_loss = -(logp * (A - A.mean()) / (A.std() + 1e-6)).mean()
        pi_loss.backward()
        phi = v_table.clone().requires_grad_(True)
        v_loss = 0.5 * ((value(phi, s) - R) ** 2).mean()
        v_loss.backward()
        with torch.no_grad():
            pi_table -= lr_pi * theta.grad  # in place, in the engine's tables
            v_table -= lr_v * phi.grad
        torch.cuda.synchronize()  # torch wrote on its stream; the next launches read on the engine's

        ends = int(((done | trunc) != 0)[:, :n].sum())
        env.rollout_closed_loop(steps, fitness=True)  # greedy validation with the new weights
        reward_sum, episodes, _, _ = env.policy_fitness()[0]
        env.policy_fitness_clear()
        print(f"round {r:2d}: {steps * n} sampled transitions, {ends} episode ends, mean V {val[:, :n].mean().item():.3f}, mean R {R.mean().item():.3f}, "
              f"critic loss {v_loss.item():.4f}; greedy validation: {int(reward_sum) / max(1, int(episodes) + n):.1f} steps per episode")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
