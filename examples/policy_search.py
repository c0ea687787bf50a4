#!/usr/bin/env python
"""Random search over a population of small policies, evaluated INSIDE the fused rollout kernel.

1024 affine CartPole policies x 1024 lanes each: one engine of 2^20 lanes, lane i plays policy i // 1024.  A generation is one
`rollout_policy_record` launch per chunk of steps: every step's action is computed from the lane's own observation in registers,
and the recorded `done` rows say which lanes finished an episode.  Fitness of a policy = how FEW episodes its 1024 lanes finished
(episodes end when the pole falls, so fewer is better); the mean episode length follows as lane-steps / finished episodes.  The
next generation keeps the best policies and perturbs them.

    python examples/policy_search.py [--policies 1024] [--lanes 1024] [--generations 5] [--steps 256]
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
    ap.add_argument("--policies", type=int, default=1024)
    ap.add_argument("--lanes", type=int, default=1024, help="lanes (parallel episode streams) per policy")
    ap.add_argument("--generations", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256, help="steps per generation")
    ap.add_argument("--chunk", type=int, default=32, help="steps per recorded launch")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n_pol, lanes = args.policies, args.lanes
    n = n_pol * lanes
    dev = "cuda:0"
    size = gymrs.policy_size(gymrs.CARTPOLE, 0)  # W[2][4], b[2]
    rng = np.random.default_rng(args.seed)
    population = rng.standard_normal((n_pol, size)).astype(np.float32)

    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET)
    stride = (n + 15) // 16 * 16
    obs = torch.empty((args.chunk, 4, stride), dtype=torch.float32, device=dev)
    act = torch.empty((args.chunk, stride), dtype=torch.uint8, device=dev)
    rew = torch.empty((args.chunk, stride), dtype=torch.float32, device=dev)
    done = torch.empty((args.chunk, stride), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    for gen in range(args.generations):
        env.reset(seed=args.seed + gen)
        env.set_policy(population, hidden=0, lanes_per_policy=lanes)
        finished = torch.zeros(n_pol, dtype=torch.int64, device=dev)
        steps = 0
        while steps < args.steps:
            k = min(args.chunk, args.steps - steps)
            env.rollout_policy_record(k, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), lane_stride=stride)
            env.sync()  # the rows were written on the engine's stream
            finished += done[:k, :n].view(k, n_pol, lanes).sum(dim=(0, 2), dtype=torch.int64)
            steps += k
        episodes = finished.cpu().numpy()
        # lanes still balancing at the end count as one (unfinished) episode each
        mean_length = steps * lanes / (episodes + lanes)
        order = np.argsort(-mean_length)
        best = order[0]
        print(f"generation {gen}: best policy {best} mean episode length {mean_length[best]:.1f} "
              f"(population median {np.median(mean_length):.1f}, {int(episodes.sum())} episodes finished)")
        elite = population[order[: max(1, n_pol // 8)]]
        children = elite[rng.integers(0, len(elite), n_pol - len(elite))]
        children = children + 0.3 * rng.standard_normal(children.shape).astype(np.float32)
        population = np.concatenate([elite, children]).astype(np.float32)
    print(f"best mean episode length: {mean_length[best]:.1f} steps (a random policy gets about 22)")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
