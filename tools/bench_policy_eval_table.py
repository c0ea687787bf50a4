#!/usr/bin/env python
"""What per-lane physics costs the episodic evaluation: gymrs_evaluate_policy with GYMRS_EVAL_LANE_PARAMS on an engine with a
parameter table against the uniform launch of the same library, in one process, on one box, taking turns
(profiles/policy_eval_table.md).

    python tools/bench_policy_eval_table.py [--policies 1024] [--lanes 1024] [--hidden 16] [--reps 9] [--json FILE]

CartPole, `policies` x `lanes` lanes, seeded normal weights with one hidden layer, E = 4, M = 200.  Four launches on one engine:
  uniform        no table, no flag: evaluate_policy_kernel<CartPoleT>
  table K=1      a one-row table equal to the engine's params, the flag: evaluate_policy_kernel<TableT<CartPoleT>> playing the SAME episodes
  table K=64     64 rows (length, masspole, force_mag scaled by uniform(0.5, 1.5)), a random index: other episodes, so the steps played
                 and the wave trips are reported next to the time
  actions+step   the 64-row table, gymrs_policy_actions + gymrs_step (GYMRS_AUTO_RESET) for `--loop-steps` steps: lane-steps/s
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a stream synchronise); the three
evaluations take turns repetition by repetition.  Also prints registers, scratch and occupancy of the evaluation kernels from the
library's code-object metadata.  Every measurement runs under its own time limit."""
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
LIMIT_S = 240

from bench_policy_rollout import kernel_source_sha16, policy_kernel_resources  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=1024)
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--loop-steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, E, M = args.policies * args.lanes, args.episodes, args.max_steps
    resources = {name: v for name, v in policy_kernel_resources(ROOT / "gym-rs_amd" / "libgymrs_amd.so").items() if "evaluate_policy_kernel" in name}
    for v in resources.values():  # waves per SIMD the 512 VGPRs of a gfx950 SIMD hold (allocation granule 8)
        if isinstance(v, dict) and "vgpr" in v:
            v["waves_per_simd"] = min(8, 512 // max(8, (v["vgpr"] + 7) // 8 * 8))

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_eval_table: no GPU visible (there is no CPU fallback)")
    kind = gymrs.CARTPOLE
    rng = np.random.default_rng(1)
    weights = rng.standard_normal((args.policies, gymrs.policy_size(kind, args.hidden))).astype(np.float32)
    base = gymrs.engine.default_params(kind)
    base.max_episode_steps = M
    rows = []
    for _ in range(args.rows):
        p = type(base).from_buffer_copy(base)
        p.length *= float(rng.uniform(0.5, 1.5))
        p.masspole *= float(rng.uniform(0.5, 1.5))
        p.force_mag *= float(rng.uniform(0.5, 1.5))
        rows.append(p)
    index = rng.integers(0, args.rows, n).astype(np.uint16)
    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "n_envs": n, "policies": args.policies,
              "lanes_per_policy": args.lanes, "hidden": args.hidden, "episodes_per_lane": E, "max_episode_steps": M, "rows": args.rows,
              "reps": args.reps, "launches": {}, "kernel_resources": resources}

    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    try:
        engines = {}
        for name in ("uniform", "table K=1", f"table K={args.rows}"):
            eng = gymrs.BatchedEngine(kind, n, flags=gymrs.AUTO_RESET, params=base)
            eng.reset(seed=0)
            eng.set_policy(weights, hidden=args.hidden, lanes_per_policy=args.lanes)
            if name == "table K=1":
                eng.set_param_table([base])
            elif name != "uniform":
                eng.set_param_table(rows)
                eng.set_param_index(index)
            engines[name] = eng

        def run(name, calls):
            eng = engines[name]
            for _ in range(calls):
                eng.evaluate_policy(E, M, 0, lane_params=name != "uniform")
            eng.sync()

        calls = {}
        for name in engines:
            run(name, 1)
            c = 1
            while True:
                t0 = time.perf_counter()
                run(name, c)
                dt = time.perf_counter() - t0
                if dt >= 0.1:
                    break
                c = max(c * 2, int(c * 0.1 / max(dt, 1e-6)) + 1)
            calls[name] = c
        times = {name: [] for name in engines}
        for _ in range(args.reps):  # taking turns
            for name in engines:
                t0 = time.perf_counter()
                run(name, calls[name])
                times[name].append((time.perf_counter() - t0) / calls[name])
        records = {}
        for name, eng in engines.items():  # what was played, and the wave trips (the price of parked lanes)
            buf = torch.zeros((E, n), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            eng.evaluate_policy(E, M, 0, lengths=buf.data_ptr(), lane_params=name != "uniform")
            rec = eng.policy_eval()
            records[name] = rec
            per_lane = (buf.cpu().numpy().view(np.uint32) & 0x7fffffff).astype(np.int64).sum(axis=0)
            played = int(per_lane.sum())
            assert played == int(rec[:, 5].sum()) and int(rec[:, 2].sum()) == E * n
            trips = np.concatenate([per_lane, np.zeros((-n) % 256, np.int64)]).reshape(-1, 256).max(axis=1)
            med = float(np.median(times[name]))
            result["launches"][name] = {"seconds_median": med, "seconds_min": min(times[name]), "seconds_max": max(times[name]), "calls_per_rep": calls[name],
                                        "lane_steps_played": played, "lane_steps_per_s": played / med, "lane_slots_stepped": int(trips.sum()) * 256,
                                        "lane_slots_per_s": int(trips.sum()) * 256 / med, "wave_trips_mean": float(trips.mean()), "wave_trips_max": int(trips.max())}
        assert np.array_equal(records["uniform"], records["table K=1"]), "a one-row table must play the uniform launch's episodes"
        # the per-step loop with the 64-row table
        eng = engines[f"table K={args.rows}"]
        act = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def loop(steps):
            for _ in range(steps):
                eng.policy_actions(act.data_ptr())
                eng.step(act.data_ptr())
            eng.sync()

        loop(10)
        loop_times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            loop(args.loop_steps)
            loop_times.append(time.perf_counter() - t0)
        med = float(np.median(loop_times))
        result["launches"]["actions+step"] = {"steps": args.loop_steps, "seconds_median": med, "seconds_min": min(loop_times), "seconds_max": max(loop_times),
                                              "lane_steps_per_s": n * args.loop_steps / med}
        for e in engines.values():
            e.close()
    finally:
        faulthandler.cancel_dump_traceback_later()

    u = result["launches"]["uniform"]
    for name, v in result["launches"].items():
        if name == "actions+step":
            print(f"{name}: {v['steps']} steps {v['seconds_median'] * 1e3:.3f} ms (min {v['seconds_min'] * 1e3:.3f}, max {v['seconds_max'] * 1e3:.3f}), "
                  f"{v['lane_steps_per_s']:.4g} lane-steps/s")
            continue
        v["time_over_uniform"] = v["seconds_median"] / u["seconds_median"]
        print(f"{name}: {v['seconds_median'] * 1e3:.3f} ms (min {v['seconds_min'] * 1e3:.3f}, max {v['seconds_max'] * 1e3:.3f}), time / uniform "
              f"{v['time_over_uniform']:.3f}; {v['lane_steps_played']} lane-steps played, {v['lane_steps_per_s']:.4g} /s; {v['lane_slots_stepped']} lane-slots, "
              f"{v['lane_slots_per_s']:.4g} /s; wave trips mean {v['wave_trips_mean']:.1f} max {v['wave_trips_max']}", flush=True)
    for name in sorted(resources):
        print(name, resources[name])
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
