#!/usr/bin/env python
"""What episodic evaluation costs: gymrs_evaluate_policy against gymrs_rollout_policy_fitness (unchanged code) over the same step
budget, in one process, on one box, alternately (profiles/policy_eval.md).

    python tools/bench_policy_eval.py [--policies 1024] [--lanes 1024] [--reps 9] [--json FILE]

Two workloads, `policies` x `lanes` lanes, affine seeded normal weights, engine flags GYMRS_AUTO_RESET | GYMRS_TIME_LIMIT with
max_episode_steps = M:
  cartpole E=4 M=200     the perf test's: random policies fall long before M, so waves leave early
  mountain_car E=4 M=20  default parameters: no episode ends before M, every lane steps E * M times: the loop's own overhead
Per workload: the time of one evaluate_policy and of one rollout_policy_fitness(E * M), median of `reps` repetitions of >= 100 ms (host
clock around calls that end in a stream synchronise; the two take turns repetition by repetition); lane-steps/s = steps really
played / time (the evaluator plays sum of L, the fixed launch n * E * M); and, from the `lengths` buffer on the host, the price of not
moving episodes between lanes: a wave runs max over its 256 lanes of (sum of L) trips, so trips * 256 summed over waves / sum of L is
the number of lane-slots stepped per lane-step played.  Also prints registers, scratch and occupancy of the evaluation kernels
from the library's code-object metadata.  Every measurement runs under its own time limit."""
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
    ap.add_argument("--policies", type=int, default=1024)
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n = args.policies * args.lanes
    resources = {name: v for name, v in policy_kernel_resources(ROOT / "gym-rs_amd" / "libgymrs_amd.so").items()
                 if "evaluate_policy_kernel" in name or "policy_eval_identity" in name}
    for v in resources.values():  # waves per SIMD the 512 VGPRs of a gfx950 SIMD hold (allocation granule 8)
        if isinstance(v, dict) and "vgpr" in v:
            v["waves_per_simd"] = min(8, 512 // max(8, (v["vgpr"] + 7) // 8 * 8))

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_eval: no GPU visible (there is no CPU fallback)")
    dev = "cuda:0"
    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "n_envs": n, "policies": args.policies,
              "lanes_per_policy": args.lanes, "reps": args.reps, "workloads": {}, "kernel_resources": resources}

    def weights(kind, n_policies, seed=1):  # tests/closed_loop_ref.make_weights, affine
        d, a = (4, 2) if kind == gymrs.CARTPOLE else (2, 3)
        rng = np.random.default_rng(seed)
        return np.stack([np.concatenate([rng.standard_normal(a * d), rng.standard_normal(a)]).astype(np.float32) for _ in range(n_policies)])

    def workload(name, kind, episodes, max_steps):
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
        try:
            p = gymrs.engine.default_params(kind)
            p.max_episode_steps = max_steps
            eng = gymrs.BatchedEngine(kind, n, flags=gymrs.AUTO_RESET | gymrs.TIME_LIMIT, params=p)
            eng.reset(seed=0)
            eng.set_policy(weights(kind, args.policies), lanes_per_policy=args.lanes)
            budget = episodes * max_steps

            def run_eval(calls):
                for _ in range(calls):
                    eng.evaluate_policy(episodes, max_steps, 0)
                eng.sync()

            def run_fit(calls):
                for _ in range(calls):
                    eng.rollout_policy_fitness(budget)
                eng.sync()

            runs = {"evaluate_policy": run_eval, "rollout_policy_fitness": run_fit}
            calls = {}
            for key, run in runs.items():
                run(1)
                c = 1
                while True:
                    t0 = time.perf_counter()
                    run(c)
                    dt = time.perf_counter() - t0
                    if dt >= 0.1:
                        break
                    c = max(c * 2, int(c * 0.1 / max(dt, 1e-6)) + 1)
                calls[key] = c
            times = {key: [] for key in runs}
            for _ in range(args.reps):  # alternately
                for key, run in runs.items():
                    t0 = time.perf_counter()
                    run(calls[key])
                    times[key].append((time.perf_counter() - t0) / calls[key])
            # what was played, and what not moving episodes between lanes costs
            buf = torch.zeros((episodes, n), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            eng.evaluate_policy(episodes, max_steps, 0, lengths=buf.data_ptr())
            rec = eng.policy_eval()
            length = (buf.cpu().numpy().view(np.uint32) & 0x7fffffff).astype(np.int64)
            per_lane = length.sum(axis=0)
            played = int(per_lane.sum())
            assert played == int(rec[:, 5].sum()) and int(rec[:, 2].sum()) == episodes * n
            pad = (-n) % 256
            trips = np.concatenate([per_lane, np.zeros(pad, np.int64)]).reshape(-1, 256).max(axis=1)
            slots = int(trips.sum()) * 256
            eng.close()
        finally:
            faulthandler.cancel_dump_traceback_later()
        med = {key: float(np.median(v)) for key, v in times.items()}
        steps = {"evaluate_policy": played, "rollout_policy_fitness": n * budget}
        out = {"episodes_per_lane": episodes, "max_episode_steps": max_steps, "lane_steps_played": played, "lane_steps_budget": n * budget,
               "mean_episode_length": played / (episodes * n), "wave_trips_mean": float(trips.mean()), "wave_trips_max": int(trips.max()),
               "lane_slots_stepped": slots, "slots_per_step_played": slots / played, "parked_share": 1.0 - played / slots,
               "eval_over_fitness_time": med["evaluate_policy"] / med["rollout_policy_fitness"]}
        for key in runs:
            out[key] = {"seconds_median": med[key], "seconds_min": min(times[key]), "seconds_max": max(times[key]),
                        "lane_steps_per_s": steps[key] / med[key]}
        out["evaluate_policy"]["lane_slots_per_s"] = slots / med["evaluate_policy"]
        result["workloads"][name] = out
        print(f"{name}: evaluate_policy {med['evaluate_policy'] * 1e3:.3f} ms (min {min(times['evaluate_policy']) * 1e3:.3f}, max "
              f"{max(times['evaluate_policy']) * 1e3:.3f}), {played / med['evaluate_policy']:.4g} lane-steps/s played, "
              f"{slots / med['evaluate_policy']:.4g} lane-slots/s; rollout_policy_fitness({budget}) {med['rollout_policy_fitness'] * 1e3:.3f} ms "
              f"(min {min(times['rollout_policy_fitness']) * 1e3:.3f}, max {max(times['rollout_policy_fitness']) * 1e3:.3f}), "
              f"{n * budget / med['rollout_policy_fitness']:.4g} lane-steps/s; time ratio {out['eval_over_fitness_time']:.3f}; mean episode length "
              f"{out['mean_episode_length']:.2f}; wave trips mean {out['wave_trips_mean']:.1f} max {out['wave_trips_max']}; slots per step played "
              f"{out['slots_per_step_played']:.3f} (parked share {out['parked_share']:.3f})", flush=True)

    workload("cartpole E=4 M=200", gymrs.CARTPOLE, 4, 200)
    workload("mountain_car E=4 M=20", gymrs.MOUNTAIN_CAR, 4, 20)
    for name in sorted(resources):
        print(name, resources[name])
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
