#!/usr/bin/env python
"""Random search ranked by exact episodic returns: every policy plays E whole episodes per lane in ONE launch.

1024 affine CartPole policies x 256 lanes each.  A generation is one `evaluate_policy` launch: every lane plays `--episodes`
complete episodes (an episode ends when the pole falls or after `--max-steps` steps), and the kernel returns per policy the exact
sum, sum of squares, minimum and maximum of the episodic returns and how the episodes ended -- no censored episodes, no estimate
from a step budget (compare examples/policy_search.py).  With common starts every policy meets the same lanes x episodes start
states, so two policies differ by what they do and not by the states they drew.  A policy is ranked by its mean return; the
standard error of that mean comes from the sum of squares.  The next generation keeps the best policies and perturbs them.

    python examples/episodic_evaluation.py [--policies 1024] [--lanes 256] [--episodes 4] [--max-steps 200] [--generations 5]
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
    ap.add_argument("--lanes", type=int, default=256, help="lanes per policy")
    ap.add_argument("--episodes", type=int, default=4, help="whole episodes per lane and generation")
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--generations", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n_pol, lanes = args.policies, args.lanes
    size = gymrs.policy_size(gymrs.CARTPOLE, 0)  # W[2][4], b[2]
    rng = np.random.default_rng(args.seed)
    population = rng.standard_normal((n_pol, size)).astype(np.float32)

    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n_pol * lanes)  # no reset: the evaluation draws its own start states
    for gen in range(args.generations):
        env.set_policy(population, hidden=0, lanes_per_policy=lanes)
        env.evaluate_policy(args.episodes, args.max_steps, seed=args.seed + 1000 * gen, common_starts=True)
        rec = env.policy_eval()  # columns: return_sum, return_sq_sum, episodes, done, truncated, steps, return_min, return_max
        count = rec[:, 2].astype(np.float64)
        mean = rec[:, 0] / count
        var = np.maximum(rec[:, 1].astype(np.uint64) / count - mean * mean, 0.0) * count / np.maximum(count - 1, 1)
        sem = np.sqrt(var / count)
        order = np.argsort(-mean)
        best = order[0]
        print(f"generation {gen}: best policy {best} mean return {mean[best]:.2f} +- {sem[best]:.2f} (min {rec[best, 6]}, max {rec[best, 7]}, "
              f"{rec[best, 4]} of {rec[best, 2]} episodes reached the limit); population median {np.median(mean):.2f}; "
              f"{int(rec[:, 5].sum())} steps played")
        elite = population[order[: max(1, n_pol // 8)]]
        children = elite[rng.integers(0, len(elite), n_pol - len(elite))]
        children = children + 0.3 * rng.standard_normal(children.shape).astype(np.float32)
        population = np.concatenate([elite, children]).astype(np.float32)
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
