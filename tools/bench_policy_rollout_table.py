#!/usr/bin/env python
"""What one fused launch under a parameter table buys and what the table costs: gymrs_rollout_closed_loop with
GYMRS_CLOSED_LOOP_LANE_PARAMS against the per-step loop it replaces and against the uniform fused launch, in one process, on one
engine per env, taking turns (profiles/policy_rollout_table.md).

    python tools/bench_policy_rollout_table.py [--policies 1024] [--lanes 1024] [--steps 100] [--rows 5] [--reps 9] [--json FILE]

CartPole and MountainCar, `policies` affine policies x `lanes` lanes, seeded normal weights, flags A | S | T.  Three variants:
  (a) closed loop     rollout_closed_loop(K, lane_params) under a table of `rows` rows and a random index: ONE launch
  (b) actions+step    K x (gymrs_policy_actions + gymrs_step) under the same table: 2K launches, every array through memory per step
  (c) uniform         gymrs_rollout_policy(K) on the same engine with the table removed: the price of the table is (a) / (c)
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a stream synchronise), with min and
max; the variants take turns repetition by repetition (the table is set / removed outside the timed region).  Also prints
registers, scratch, spills and waves per SIMD of the TableT closed-loop kernel families from the library's code-object metadata.
Every measurement runs under its own time limit."""
from __future__ import annotations

import argparse
import faulthandler
import importlib
import json
import re
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
LIMIT_S = 120  # per measurement

from bench_policy_rollout import kernel_source_sha16, policy_kernel_resources  # noqa: E402


def families(resources: dict) -> dict:
    """The TableT closed-loop kernels grouped per family (kernel, env, lanes per work-item, recording): ranges over the flag sets"""
    out = {}
    for name, v in resources.items():
        m = re.match(r"(rollout_policy(?:_fitness)?_kernel)<TableT<(\w+)T>, (\d+), \d+u(?:, (true|false))?>", name)
        if not m or not isinstance(v, dict):
            continue
        key = f"{m.group(1)}<TableT<{m.group(2)}T>, {m.group(3)}{', recording' if m.group(4) == 'true' else ''}>"
        f = out.setdefault(key, {"kernels": 0, "vgpr": [], "sgpr": [], "scratch_bytes": [], "vgpr_spill": [], "sgpr_spill": []})
        f["kernels"] += 1
        for k in ("vgpr", "sgpr", "scratch_bytes", "vgpr_spill", "sgpr_spill"):
            f[k].append(v[k])
    for f in out.values():
        for k in ("vgpr", "sgpr", "scratch_bytes", "vgpr_spill", "sgpr_spill"):
            f[k] = [min(f[k]), max(f[k])]
        f["waves_per_simd"] = min(8, 512 // max(8, (f["vgpr"][1] + 7) // 8 * 8))  # the 512 VGPRs of a gfx950 SIMD, allocation granule 8
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=1024)
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, K = args.policies * args.lanes, args.steps
    fams = families(policy_kernel_resources(ROOT / "gym-rs_amd" / "libgymrs_amd.so"))

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout_table: no GPU visible (there is no CPU fallback)")
    flags = gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT
    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "n_envs": n, "policies": args.policies,
              "lanes_per_policy": args.lanes, "steps": K, "rows": args.rows, "flags": flags, "reps": args.reps, "envs": {}, "kernel_families": fams}
    scaled = {gymrs.CARTPOLE: ("length", "masspole", "force_mag", "gravity"), gymrs.MOUNTAIN_CAR: ("force", "gravity")}
    for env, kind in (("cartpole", gymrs.CARTPOLE), ("mountain_car", gymrs.MOUNTAIN_CAR)):
        rng = np.random.default_rng(1)
        weights = rng.standard_normal((args.policies, gymrs.policy_size(kind, 0))).astype(np.float32)
        base = gymrs.engine.default_params(kind)
        rows = []
        for _ in range(args.rows):
            p = type(base).from_buffer_copy(base)
            for f in scaled[kind]:
                setattr(p, f, getattr(p, f) * float(rng.uniform(0.5, 1.5)))
            rows.append(p)
        index = rng.integers(0, args.rows, n).astype(np.uint16)
        eng = gymrs.BatchedEngine(kind, n, flags=flags, params=base)
        eng.reset(seed=0)
        eng.set_policy(weights, hidden=0, lanes_per_policy=args.lanes)
        act = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def table(on):
            if on:
                eng.set_param_table(rows)
                eng.set_param_index(index)
            else:
                eng.set_param_table(None)
                eng.set_params(base)
            eng.sync()

        def closed_loop(calls):
            for _ in range(calls):
                eng.rollout_closed_loop(K, lane_params=True)
            eng.sync()

        def actions_step(calls):
            for _ in range(calls * K):
                eng.policy_actions(act.data_ptr())
                eng.step(act.data_ptr())
            eng.sync()

        def uniform(calls):
            for _ in range(calls):
                eng.rollout_policy(K)
            eng.sync()

        variants = {"closed loop": (closed_loop, True), "actions+step": (actions_step, True), "uniform": (uniform, False)}
        calls, times = {}, {name: [] for name in variants}
        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
        try:
            for name, (run, on) in variants.items():  # warm-up, and how many calls make 100 ms
                table(on)
                run(1)
                c = 1
                while True:
                    t0 = time.perf_counter()
                    run(c)
                    dt = time.perf_counter() - t0
                    if dt >= 0.1:
                        break
                    c = max(c * 2, int(c * 0.1 / max(dt, 1e-6)) + 1)
                calls[name] = c
        finally:
            faulthandler.cancel_dump_traceback_later()
        for _ in range(args.reps):  # taking turns
            for name, (run, on) in variants.items():
                faulthandler.dump_traceback_later(LIMIT_S, exit=True)
                try:
                    table(on)
                    t0 = time.perf_counter()
                    run(calls[name])
                    times[name].append((time.perf_counter() - t0) / calls[name])
                finally:
                    faulthandler.cancel_dump_traceback_later()
        eng.close()
        out = {}
        for name, ts in times.items():
            med = float(np.median(ts))
            out[name] = {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name],
                         "lane_steps_per_s": n * K / med}
        out["closed_loop_over_actions_step"] = out["closed loop"]["seconds_median"] / out["actions+step"]["seconds_median"]
        out["closed_loop_over_uniform"] = out["closed loop"]["seconds_median"] / out["uniform"]["seconds_median"]
        result["envs"][env] = out
        for name in variants:
            v = out[name]
            print(f"{env} {name}: {K} steps {v['seconds_median'] * 1e3:.3f} ms (min {v['seconds_min'] * 1e3:.3f}, max {v['seconds_max'] * 1e3:.3f}), "
                  f"{v['lane_steps_per_s']:.4g} lane-steps/s", flush=True)
        print(f"{env}: (a) / (b) = {out['closed_loop_over_actions_step']:.4f}, (a) / (c) = {out['closed_loop_over_uniform']:.3f}", flush=True)
    for name in sorted(fams):
        print(name, fams[name])
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
