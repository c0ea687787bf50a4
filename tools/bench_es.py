#!/usr/bin/env python
"""One generation step of evolution strategies on the device against the same step through the host (profiles/evolution_strategies.md).

    python tools/bench_es.py [--reps 5] [--json FILE] [--only device]

Shapes: (P = 2^20, hidden 0: S = 10) and (P = 4096, hidden 64: S = 450), CartPole, one lane per policy.
  device  es_step(adam=True, max_norm=10) after ONE evaluate_policy: the utilities passes, the gradient and the fused update and
          population, no synchronisation between calls (the step does not depend on the values, so the evaluation is not repeated;
          the table is handed over again by passing the engine's own utilities row from the second call on -- `device_table` times
          the calls that read the records, re-arming the table with a 1-step evaluation whose cost `evaluate` gives on its own).
  host    what examples/policy_search.py does per generation: policy_eval() to the host (synchronising), a numpy update of the
          same kind (standardised returns, antithetic gradient estimate from a noise matrix kept on the host, SGD, the next
          population) and set_policy (synchronising).
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max,
taking turns.  `--only device` runs the device steps alone, a fixed number of times, for a kernel trace."""
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
LIMIT_S = 120  # per measurement
SHAPES = [(1 << 20, 0), (4096, 64)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, choices=["device"])
    args = ap.parse_args()

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_es: no GPU visible (there is no CPU fallback)")

    def timed(run, calls):
        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
        try:
            t0 = time.perf_counter()
            run(calls)
            return time.perf_counter() - t0
        finally:
            faulthandler.cancel_dump_traceback_later()

    def calibrate(run):
        timed(run, 1)
        c = 1
        while (dt := timed(run, c)) < 0.1:
            c = max(c * 2, int(c * 0.1 / max(dt, 1e-6)) + 1)
        return c

    def measure(variants):
        calls = {name: calibrate(run) for name, run in variants.items()}
        times = {name: [] for name in variants}
        for _ in range(args.reps):  # taking turns
            for name, run in variants.items():
                times[name].append(timed(run, calls[name]) / calls[name])
        return {name: {"seconds_median": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name]}
                for name, ts in times.items()}

    result = {"gpu": torch.cuda.get_device_name(0), "reps": args.reps, "cases": {}}
    sigma = 0.1
    for P, hidden in SHAPES:
        size = gymrs.policy_size(gymrs.CARTPOLE, hidden)
        rng = np.random.default_rng(1)
        centre = (0.1 * rng.standard_normal(size)).astype(np.float32)
        eng = gymrs.BatchedEngine(gymrs.CARTPOLE, P, flags=gymrs.AUTO_RESET)
        eng.es_init(centre, n_policies=P, sigma=sigma, seed=1, hidden=hidden)
        eng.evaluate_policy(1, max_episode_steps=32, seed=0)
        step = dict(adam=True, lr=0.01, grad_scale=2.0**-24 / (P * sigma), max_norm=10.0)
        eng.es_step(**step)
        eng.sync()
        own_row = eng.es_utilities_ptr()[0]

        def device(calls):  # the caller's-utilities route: gradient + update and population
            for _ in range(calls):
                eng.es_step(utilities=own_row, **step)
            eng.sync()

        def evaluate(calls):
            for _ in range(calls):
                eng.evaluate_policy(1, max_episode_steps=1, seed=0)
            eng.sync()

        def device_table(calls):  # the whole step: three utilities passes too (and the 1-step evaluation that re-arms the table)
            for _ in range(calls):
                eng.evaluate_policy(1, max_episode_steps=1, seed=0)
                eng.es_step(**step)
            eng.sync()

        if args.only == "device":
            device_table(20)
            eng.close()
            continue

        noise = rng.standard_normal((P // 2, size)).astype(np.float32)
        theta = centre.copy()

        def host(calls):
            nonlocal theta
            for _ in range(calls):
                rec = eng.policy_eval()  # synchronising copy of P x 64 bytes
                F = rec[:, 0] / np.maximum(rec[:, 2], 1)
                u = ((F - F.mean()) / (F.std() + 1e-12)).astype(np.float32)
                theta = theta + np.float32(0.01 / (P * sigma)) * ((u[0::2] - u[1::2]) @ noise)
                pop = np.empty((P, size), np.float32)
                pop[0::2], pop[1::2] = theta + sigma * noise, theta - sigma * noise
                eng.set_policy(pop, hidden=hidden, lanes_per_policy=1)  # synchronising copy of P x S floats
                eng.evaluate_policy(1, max_episode_steps=1, seed=0)  # (set_policy discards the table: the next read needs one)

        out = measure({"device": device, "evaluate": evaluate, "device_table": device_table, "host": host})
        whole = out["device_table"]["seconds_median"] - out["evaluate"]["seconds_median"]
        host_only = out["host"]["seconds_median"] - out["evaluate"]["seconds_median"]
        out["device_step_seconds"], out["host_step_seconds"], out["host_over_device"] = whole, host_only, host_only / whole
        out["philox_blocks_per_step"] = P * size  # P/2 * S in the gradient and again in the population
        for name in ("device", "evaluate", "device_table", "host"):
            t = out[name]
            print(f"P={P} S={size} | {name}: {t['seconds_median'] * 1e6:.1f} us (min {t['seconds_min'] * 1e6:.1f}, max {t['seconds_max'] * 1e6:.1f})", flush=True)
        print(f"P={P} S={size} | device step {whole * 1e6:.1f} us, host step {host_only * 1e6:.1f} us: host / device = {out['host_over_device']:.1f}", flush=True)
        result["cases"][f"P={P},S={size}"] = out
        eng.close()
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
