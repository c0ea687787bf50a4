#!/usr/bin/env python
"""Whole transitions from one fused launch: the Q-learning loop of epsilon_greedy_collection.py with the truncated steps kept.

`rollout_transitions(K, record=..., final_obs=..., start_obs=..., explore=True)` writes the record rows of `rollout_closed_loop` and,
for every step that ended an episode, the observation the episode ended in (the record's `obs` row holds the re-armed state there).
The successor of step k is therefore `where(ended[k], final_obs[k], obs[k])` and its predecessor `obs[k - 1]` (`start_obs` for k = 0):
all K transitions of every lane are usable.  A terminated step does not bootstrap; a truncated one bootstraps from its final
observation, which is what the time limit asks for.  Under a short time limit most episodes of a decent policy end by truncation,
and the loop that drops those steps (the older example) loses them all; this one prints how many that would have been.

    python examples/transition_collection.py [--lanes 4096] [--steps 64] [--rounds 12] [--limit 50]
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
    ap.add_argument("--limit", type=int, default=50, help="max_episode_steps")
    ap.add_argument("--epsilon", type=float, default=0.5, help="of the first round; halves every third round")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n, steps, dev = args.lanes, args.steps, "cuda:0"
    gamma, lr, explore_seed = 0.97, 0.05, 1234
    rng = np.random.default_rng(args.seed)
    weights = (0.1 * rng.standard_normal(gymrs.policy_size(gymrs.CARTPOLE, 0))).astype(np.float32)  # W[2][4], b[2]

    params = gymrs.engine.default_params(gymrs.CARTPOLE)
    params.max_episode_steps = args.limit
    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT, params=params)
    env.reset(seed=args.seed)
    env.set_policy(weights, hidden=0, lanes_per_policy=n)

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
        env.set_exploration(explore_seed, epsilon=args.epsilon * 0.5 ** (r // 3))
        env.rollout_transitions(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), explore=True)
        env.sync()

        # all K transitions (s, a, r, s', done): s' is the final observation where the step ended an episode
        ended = ((done | trunc) != 0)[:, None, :n]
        s = torch.cat([start[None, :, :n], obs[:-1, :, :n]])
        s2 = torch.where(ended, final[:, :, :n], obs[:, :, :n])
        w = torch.from_numpy(weights[:8].reshape(2, 4)).to(dev)
        b = torch.from_numpy(weights[8:]).to(dev)
        a = act[:, :n].long()
        q = torch.einsum("aj,kjn->kan", w, s) + b[None, :, None]
        q2 = torch.einsum("aj,kjn->kan", w, s2) + b[None, :, None]
        target = rew[:, :n] + gamma * q2.max(dim=1).values * (done[:, :n] == 0)  # a truncated step bootstraps, a terminated one does not
        td = target - q.gather(1, a[:, None, :]).squeeze(1)
        onehot = torch.nn.functional.one_hot(a, 2).permute(0, 2, 1).float()  # [K][2][n]
        grad_w = torch.einsum("kn,kan,kjn->aj", td, onehot, s) / td.numel()
        grad_b = torch.einsum("kn,kan->a", td, onehot) / td.numel()
        weights = torch.cat([(w + lr * grad_w).reshape(-1), b + lr * grad_b]).cpu().numpy().astype(np.float32)
        n_trunc, n_done = int((trunc[:, :n] != 0).sum()), int((done[:, :n] != 0).sum())
        torch.cuda.synchronize()
        env.set_policy(weights, hidden=0, lanes_per_policy=n)

        env.rollout_closed_loop(steps, fitness=True)  # greedy validation
        _, episodes, _, _ = env.policy_fitness()[0]
        print(f"round {r:2d}: {steps * n} transitions, {n_done} terminated, {n_trunc} truncated and bootstrapped from final_obs "
              f"(dropping them, and step 0 of every lane, would have lost {n_trunc + n} = {(n_trunc + n) / (steps * n):.1%}); "
              f"mean |TD| {float(td.abs().mean()):.3f}; greedy validation: {int(episodes)} episodes ended")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
