#!/usr/bin/env python
"""What the per-policy fitness counters cost: gymrs_rollout_policy_fitness against gymrs_rollout_policy (unchanged code), in one
process, on one box, alternately (profiles/policy_fitness.md).

    python tools/bench_policy_fitness.py [--n-envs 1048576] [--k 256] [--reps 9] [--json FILE]

CartPole, GYMRS_AUTO_RESET | GYMRS_TRACK_STATS, K steps per launch, hidden 0 and 16, three layouts: one policy (uniform weights),
1024 policies x 1024 lanes (uniform, one record per wave) and 4096 policies with lanes_per_policy = 1 (gathered: per-lane counters
and up to four 64-bit adds per lane and launch); then the 1024 x 1024 layout, affine, at 8 lanes per work-item and with
GYMRS_TIME_LIMIT | GYMRS_FINAL_OBS added (the flag sets whose combined kernels carry scratch).  Every figure: median of `reps` repetitions of >= 100 ms, host clock around work
that ends in a stream synchronise; the two calls take turns repetition by repetition.  Also prints the register and scratch figures
of the fitness kernels from the library's code-object metadata.  Every measurement runs under its own time limit."""
from __future__ import annotations

import argparse
import faulthandler
import importlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
STEP_LIMIT_S = 120

from bench_policy_rollout import kernel_source_sha16, policy_kernel_resources  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, k = args.n_envs, args.k
    resources = {name: v for name, v in policy_kernel_resources(ROOT / "gym-rs_amd" / "libgymrs_amd.so").items() if "fitness" in name}

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_fitness: no GPU visible (there is no CPU fallback)")
    flags = gymrs.AUTO_RESET | gymrs.TRACK_STATS
    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "n_envs": n, "k": k, "reps": args.reps,
              "rates": {}, "kernel_resources": resources}

    def weights(hidden, n_policies, seed=1):  # as tools/bench_policy_rollout.py
        rng = np.random.default_rng(seed)
        d, a = 4, 2
        rows = []
        for _ in range(n_policies):
            if hidden == 0:
                parts = [rng.standard_normal(a * d), rng.standard_normal(a)]
            else:
                parts = [rng.standard_normal(hidden * d) / np.sqrt(d), rng.standard_normal(hidden) / np.sqrt(d),
                         rng.standard_normal(a * hidden) / np.sqrt(hidden), rng.standard_normal(a) / np.sqrt(hidden)]
            rows.append(np.concatenate(parts).astype(np.float32))
        return np.stack(rows)

    def pair(name, hidden, n_pol, lpp, flags=flags, lanes_per_thread=None):
        """Two engines from the same reset with the same set: one steps with rollout_policy, the other with rollout_policy_fitness"""
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
        try:
            engines = []
            for _ in range(2):
                e = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=flags, lanes_per_thread=lanes_per_thread)
                e.reset(seed=0)
                e.set_policy(weights(hidden, n_pol), hidden=hidden, lanes_per_policy=lpp)
                engines.append(e)
            plain, fit = engines

            def run_plain(calls):
                for _ in range(calls):
                    plain.rollout_policy(k)
                plain.sync()

            def run_fit(calls):
                for _ in range(calls):
                    fit.rollout_policy_fitness(k)
                fit.sync()

            run_plain(1)
            run_fit(1)
            calls = 1
            while True:  # size one repetition (both engines take the same steps, so their states can be compared at the end)
                t0 = time.perf_counter()
                run_plain(calls)
                dt = time.perf_counter() - t0
                run_fit(calls)
                if dt >= 0.1:
                    break
                calls = max(calls * 2, int(calls * 0.1 / max(dt, 1e-6)) + 1)
            rates = {"rollout_policy": [], "rollout_policy_fitness": []}
            for _ in range(args.reps):  # alternately
                for key, run in (("rollout_policy", run_plain), ("rollout_policy_fitness", run_fit)):
                    t0 = time.perf_counter()
                    run(calls)
                    rates[key].append(calls * n * k / (time.perf_counter() - t0))
            same = np.array_equal(plain.get_state().view(np.uint32), fit.get_state().view(np.uint32))
            episodes = int(fit.policy_fitness()[:, 1].sum())
            for e in engines:
                e.close()
        finally:
            faulthandler.cancel_dump_traceback_later()
        med = {key: float(np.median(v)) for key, v in rates.items()}
        result["rates"][name] = {key: {"median": med[key], "min": min(v), "max": max(v)} for key, v in rates.items()}
        result["rates"][name]["fitness_over_plain"] = med["rollout_policy_fitness"] / med["rollout_policy"]
        print(f"{name:44s} rollout_policy {med['rollout_policy']:.4g} (min {min(rates['rollout_policy']):.4g}, max {max(rates['rollout_policy']):.4g})  "
              f"fitness {med['rollout_policy_fitness']:.4g} (min {min(rates['rollout_policy_fitness']):.4g}, max {max(rates['rollout_policy_fitness']):.4g})  "
              f"ratio {med['rollout_policy_fitness'] / med['rollout_policy']:.4f}  same state {same}  episodes counted {episodes}", flush=True)

    for hidden in (0, 16):
        pair(f"H={hidden} uniform P=1", hidden, 1, 1)
        pair(f"H={hidden} uniform P=1024 x 1024 lanes", hidden, 1024, 1024)
        pair(f"H={hidden} gathered P=4096 lanes_per_policy=1", hidden, 4096, 1)
    full = flags | gymrs.TIME_LIMIT | gymrs.FINAL_OBS
    pair("H=0 uniform P=1024 x 1024 lanes, 8 lanes per work-item", 0, 1024, 1024, lanes_per_thread=8)
    pair("H=0 uniform P=1024 x 1024 lanes, A|S|T|F", 0, 1024, 1024, flags=full)
    pair("H=0 uniform P=1024 x 1024 lanes, A|S|T|F, 8 lanes per work-item", 0, 1024, 1024, flags=full, lanes_per_thread=8)
    if resources and "error" not in resources:
        for name in sorted(resources):
            print(name, resources[name])
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
