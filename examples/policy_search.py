#!/usr/bin/env python
"""Random search over a population of small policies, evaluated INSIDE the fused rollout kernel.

1024 affine CartPole policies x 1024 lanes each: one engine of 2^20 lanes, lane i plays policy i // 1024.  A generation is ONE
`rollout_policy_fitness` launch: every step's action is computed from the lane's own observation in registers, and the kernel
counts per policy what its lanes earned and how many episodes they finished (no trajectory buffers).  Fitness of a policy = how
FEW episodes its 1024 lanes finished (episodes end when the pole falls, so fewer is better); the mean episode length follows as
lane-steps / finished episodes.  The next generation keeps the best policies and perturbs them.

    python examples/policy_search.py [--policies 1024] [--lanes 1024] [--generations 5] [--steps 256]
"""
from __future__ import annotations

import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
gymrs = importlib.import_module("gym-rs_amd")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=1024)
    ap.add_argument("--lanes", type=int, default=1024, help="lanes (parallel episode streams) per policy")
    ap.add_argument("--generations", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256, help="steps per generation")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n_pol, lanes = args.policies, args.lanes
    n = n_pol * lanes
    size = gymrs.policy_size(gymrs.CARTPOLE, 0)  # W[2][4], b[2]
    rng = np.random.default_rng(args.seed)
    population = rng.standard_normal((n_pol, size)).astype(np.float32)

    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET)

    for gen in range(args.generations):
        env.reset(seed=args.seed + gen)
        env.set_policy(population, hidden=0, lanes_per_policy=lanes)
        steps = args.steps
        env.rollout_policy_fitness(steps)  # (set_policy starts every generation from zeroed counters)
        episodes = env.policy_fitness()[:, 1]  # columns: reward_sum, episodes, done, truncated (synchronising)
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
