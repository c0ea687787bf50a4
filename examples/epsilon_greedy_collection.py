#!/usr/bin/env python
"""Epsilon-greedy data collection for a learner: explore inside the fused launch, validate greedily, know which actions explored.

A linear Q-function on CartPole, Q(s, a) = W[a] . s + b[a], IS an affine policy of the engine (its argmax is the greedy action), so
the engine plays it inside the kernel.  Every round
  1. collects K steps of every lane in ONE launch with `rollout_closed_loop(K, explore=True, record=...)`: the action of a step is
     random with probability epsilon (decaying round by round) and the argmax otherwise; the record's `actions` rows hold the action
     taken;
  2. recovers which recorded actions were exploratory with `explore_draw` from (global lane id, tick) alone -- no extra trajectory
     row -- and checks on a few lanes that an explored action is the draw's random action;
  3. takes one semi-gradient Q-learning step on the batch (torch, on the device buffers the kernel wrote) and installs the new
     weights with `set_policy` (the exploration settings survive it);
  4. validates the new policy with a greedy launch (`fitness=True`, no `explore`): fewer episodes ended = longer balancing.

    python examples/epsilon_greedy_collection.py [--lanes 4096] [--steps 64] [--rounds 12]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64, help="K: steps per launch")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--epsilon", type=float, default=0.5, help="of the first round; halves every third round")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n, steps, dev = args.lanes, args.steps, "cuda:0"
    gamma, lr, explore_seed = 0.97, 0.05, 1234
    rng = np.random.default_rng(args.seed)
    weights = (0.1 * rng.standard_normal(gymrs.policy_size(gymrs.CARTPOLE, 0))).astype(np.float32)  # W[2][4], b[2]

    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT)
    env.reset(seed=args.seed)
    env.set_policy(weights, hidden=0, lanes_per_policy=n)

    stride = (n + 15) // 16 * 16
    obs = torch.empty((steps, 4, stride), dtype=torch.float32, device=dev)
    act = torch.empty((steps, stride), dtype=torch.uint8, device=dev)
    rew = torch.empty((steps, stride), dtype=torch.float32, device=dev)
    done = torch.empty((steps, stride), dtype=torch.uint8, device=dev)
    trunc = torch.empty((steps, stride), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                  lane_stride=stride)
    probe = np.arange(0, n, max(1, n // 32))[:32]  # the lanes whose explored mask is recomputed on the host

    for r in range(args.rounds):
        epsilon = args.epsilon * 0.5 ** (r // 3)
        env.set_exploration(explore_seed, epsilon=epsilon)
        _, threshold = env.exploration()  # epsilon on the grid of 1 / 65536
        t0 = env.tick()[0]                # row k of the record is the step from tick t0 + k
        env.rollout_closed_loop(steps, explore=True, record=record)
        env.sync()

        # which recorded actions were exploratory: recomputed from (global lane id, tick)
        explored, random_action = gymrs.explore_draw(explore_seed, threshold, 2, probe[None, :], t0 + np.arange(steps)[:, None])
        taken = act[:, :n].cpu().numpy()[:, probe]
        assert np.array_equal(taken[explored], random_action[explored])  # an explored step took the draw's action

        # one semi-gradient Q-learning step on the transitions (obs[k - 1], act[k], rew[k], obs[k]); truncated steps are left out
        # (their successor is a reset state), terminated ones do not bootstrap
        w = torch.from_numpy(weights[:8].reshape(2, 4)).to(dev)
        b = torch.from_numpy(weights[8:]).to(dev)
        s, s2 = obs[:-1, :, :n], obs[1:, :, :n]
        a = act[1:, :n].long()
        q = torch.einsum("aj,kjn->kan", w, s) + b[None, :, None]
        q2 = torch.einsum("aj,kjn->kan", w, s2) + b[None, :, None]
        target = rew[1:, :n] + gamma * q2.max(dim=1).values * (done[1:, :n] == 0)
        td = (target - q.gather(1, a[:, None, :]).squeeze(1)) * (trunc[1:, :n] == 0)
        onehot = torch.nn.functional.one_hot(a, 2).permute(0, 2, 1).float()  # [K - 1][2][n]
        grad_w = torch.einsum("kn,kan,kjn->aj", td, onehot, s) / td.numel()
        grad_b = torch.einsum("kn,kan->a", td, onehot) / td.numel()
        weights = torch.cat([(w + lr * grad_w).reshape(-1), b + lr * grad_b]).cpu().numpy().astype(np.float32)
        torch.cuda.synchronize()
        env.set_policy(weights, hidden=0, lanes_per_policy=n)  # keeps the exploration settings, discards the fitness table

        # greedy validation: the same call without `explore`
        env.rollout_closed_loop(steps, fitness=True)
        reward_sum, episodes, _, _ = env.policy_fitness()[0]
        print(f"round {r:2d}: epsilon {threshold / 65536:.4f} ({explored.mean():.1%} of {explored.size} probed steps explored), "
              f"mean |TD| {float(td.abs().mean()):.3f}; greedy validation: {int(episodes)} episodes ended in {steps} x {n} lane-steps "
              f"(mean length {steps * n / max(1, int(episodes)):.1f})")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
