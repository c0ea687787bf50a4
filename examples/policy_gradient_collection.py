#!/usr/bin/env python
"""On-policy collection for a policy-gradient learner from one fused launch: REINFORCE on CartPole with an affine policy.

`set_sampling(seed, temperature=1)` and `rollout_transitions(K, ..., sample=True)` play a ~ softmax(logits / temperature) inside the
kernel, every draw keyed (seed, global lane id, engine tick), and write whole transitions.  The launch writes no probability row:
the record layouts are pinned, and the learner holds the weights the launch played, so it recomputes log pi(a|s) from the `obs`
rows -- here in torch, with autograd supplying the gradient.  (`gymrs.sample_draw` is the kernel's rule as host code, for a caller
that wants the kernel's own f32 probabilities.)  The update is written straight into the engine's weight table through
`policy_weights_ptr` (zero-copy), so the next launch plays the new policy without a `set_policy`.

    python examples/policy_gradient_collection.py [--lanes 4096] [--steps 64] [--rounds 12] [--limit 100]
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
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n, steps, dev = args.lanes, args.steps, "cuda:0"
    gamma, lr, sample_seed = 0.97, 0.5, 4321
    rng = np.random.default_rng(args.seed)
    weights = (0.1 * rng.standard_normal(gymrs.policy_size(gymrs.CARTPOLE, 0))).astype(np.float32)  # W[2][4], b[2]

    params = gymrs.engine.default_params(gymrs.CARTPOLE)
    params.max_episode_steps = args.limit
    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT, params=params)
    env.reset(seed=args.seed)
    env.set_policy(weights, hidden=0, lanes_per_policy=n)
    env.set_sampling(sample_seed, temperature=args.temperature)
    ptr, count = env.policy_weights_ptr()
    table = torch.as_tensor(DeviceFloats(ptr, count), device=dev)  # the engine's own weights

    stride = (n + 15) // 16 * 16
    obs = torch.empty((steps, 4, stride), dtype=torch.float32, device=dev)
    act = torch.empty((steps, stride), dtype=torch.uint8, device=dev)
    rew = torch.empty((steps, stride), dtype=torch.float32, device=dev)
    done = torch.empty((steps, stride), dtype=torch.uint8, device=dev)
    trunc = torch.empty((steps, stride), dtype=torch.uint8, device=dev)
    final = torch.zeros((steps, 4, stride), dtype=torch.float32, device=dev)  # only ended lane-steps are ever written
    start = torch.empty((4, stride), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                  lane_stride=stride)

    for r in range(args.rounds):
        env.rollout_transitions(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), sample=True)
        env.sync()

        # the K transitions of every lane: s is the observation the action was drawn from
        s = torch.cat([start[None, :, :n], obs[:-1, :, :n]])
        a = act[:, :n].long()
        ended = ((done | trunc) != 0)[:, :n]
        theta = table.clone().requires_grad_(True)
        w, b = theta[:8].reshape(2, 4), theta[8:]
        logits = torch.einsum("aj,kjn->kan", w, s) + b[None, :, None]
        logp = torch.log_softmax(logits / args.temperature, dim=1).gather(1, a[:, None, :]).squeeze(1)  # log pi(a|s), recomputed
        # reward-to-go inside the window, cut where an episode ended; normalised as a baseline
        ret = torch.zeros((steps, n), device=dev)
        run = torch.zeros(n, device=dev)
        for k in range(steps - 1, -1, -1):
            run = rew[k, :n] + gamma * run * (~ended[k])
            ret[k] = run
        adv = (ret - ret.mean()) / (ret.std() + 1e-6)
        loss = -(logp * adv).mean()
        loss.backward()
        with torch.no_grad():
            table -= lr * theta.grad  # in place, in the engine's table
        torch.cuda.synchronize()  # torch wrote on its stream; the next launch reads on the engine's

        env.rollout_closed_loop(steps, fitness=True)  # greedy validation with the new weights
        reward_sum, episodes, _, _ = env.policy_fitness()[0]
        env.policy_fitness_clear()
        print(f"round {r:2d}: {steps * n} sampled transitions, {int(ended.sum())} episode ends, mean log pi {logp.mean().item():.3f}, "
              f"loss {loss.item():.4f}; greedy validation: {int(reward_sum) / max(1, int(episodes) + n):.1f} steps per episode")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
