#!/usr/bin/env python
"""gymrs_es_ranks against its torch restatement on the same stream and the same table (profiles/es_ranks.md).

    python tools/bench_es_ranks.py [--reps 7] [--json FILE]

P = 256, 4096, 2^16, 2^20, CartPole, one lane per policy.  The table holds CartPole-like returns with realistic ties: four episodes
per policy, integer returns, a quarter of the population at the cap of 500.
  ranks     eng.es_ranks(u, rank2): one launch up to 4096 policies, two above
  torch     F from the table's columns, torch.sort, two torch.searchsorted and the arithmetic of the rule, on the engine's stream
  evaluate  the evaluate_policy(1) of a real population that precedes either in a generation (timed first, on its own)
Each time is the median of `reps` repetitions of >= 50 ms (host clock around calls that end in a synchronise), with min and max;
ranks and torch take turns.  Before anything is timed the two rows are compared bit for bit."""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SIZES = [256, 4096, 1 << 16, 1 << 20]


class DeviceRow:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_es_ranks: no GPU visible (there is no CPU fallback)")

    def timed(run, calls):
        t0 = time.perf_counter()
        run(calls)
        return (time.perf_counter() - t0) / calls

    def measure(variants):
        calls = {}
        for name, run in variants.items():
            run(3)  # warm
            calls[name] = max(1, int(0.05 / timed(run, 3)) + 1)
        times = {name: [] for name in variants}
        for _ in range(args.reps):  # taking turns
            for name, run in variants.items():
                times[name].append(timed(run, calls[name]))
        return {name: {"seconds_median": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name]}
                for name, ts in times.items()}

    result = {"gpu": torch.cuda.get_device_name(0), "reps": args.reps, "cases": {}}
    for P in SIZES:
        rng = np.random.default_rng(P)
        eng = gymrs.BatchedEngine(gymrs.CARTPOLE, P, flags=gymrs.AUTO_RESET)
        eng.es_init((0.1 * rng.standard_normal(10)).astype(np.float32), n_policies=P, sigma=0.1, seed=1)

        def evaluate(calls):
            for _ in range(calls):
                eng.evaluate_policy(1, seed=0)
            eng.sync()

        out = measure({"evaluate": evaluate})
        stream = torch.cuda.ExternalStream(eng.stream)
        rec = np.zeros((P, 8), np.int64)
        rec[:, 0], rec[:, 2] = np.where(rng.random(P) < 0.25, 2000, rng.integers(32, 800, P)), 4
        with torch.cuda.stream(stream):
            table = torch.as_tensor(DeviceRow(eng.policy_eval_ptr()[0], P * 8, "<i8"), device="cuda").view(P, 8)
            table.copy_(torch.from_numpy(rec))
            u, rank2 = torch.zeros(P, dtype=torch.float32, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
        eng.sync()

        def torch_once():
            valid = table[:, 2] > 0
            F = torch.where(valid, table[:, 0].double() / table[:, 2].double(), torch.inf)
            ordered, n = torch.sort(F).values, valid.sum()
            r2 = torch.searchsorted(ordered, F, right=False) + torch.searchsorted(ordered, F, right=True) - 1
            return torch.where(valid & (n > 1), ((r2 - (n - 1)).double() / (2 * (n - 1)).double()).float(), 0.0)

        def ranks(calls):
            for _ in range(calls):
                eng.es_ranks(u.data_ptr(), rank2.data_ptr())
            eng.sync()

        def restated(calls):
            with torch.cuda.stream(stream):
                for _ in range(calls):
                    torch_once()
            eng.sync()

        ranks(1)
        with torch.cuda.stream(stream):
            same = bool((torch_once().view(torch.int32) == u.view(torch.int32)).all())
        if not same:
            raise SystemExit(f"bench_es_ranks: P={P}: the kernel and the torch restatement differ")
        out.update(measure({"ranks": ranks, "torch": restated}))
        out["torch_over_ranks"] = out["torch"]["seconds_median"] / out["ranks"]["seconds_median"]
        for name in ("evaluate", "ranks", "torch"):
            t = out[name]
            print(f"P={P} | {name}: {t['seconds_median'] * 1e6:.1f} us (min {t['seconds_min'] * 1e6:.1f}, max {t['seconds_max'] * 1e6:.1f})", flush=True)
        result["cases"][f"P={P}"] = out
        eng.close()
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
