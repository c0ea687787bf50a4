#!/usr/bin/env python
"""One critic epoch and one advantage normalisation over a record: gymrs_value_gradient and gymrs_normalize_advantages against what
they replace (profiles/value_gradient.md, profiles/normalize.md).  One process, taking turns:

    python tools/bench_value_gradient.py [--n-envs 1048576] [--steps 64] [--reps 5] [--json FILE]

CartPole, one critic for all lanes, H = 0 and 64, a synthetic record (standard normal observations, returns and old values).
  value      value_gradient(K, record, start_obs, returns, old_values, clip 0.2 -> values, grad, excluded, sums, counts)
  plain      the same without old_values
  composed   what an epoch did without it: torch.sub(values, returns) into a coefficient row, policy_gradient(critic) with that row,
             then advantages(critic) for the values row of the next epoch (two synchronisations: torch runs on its own stream)
  single     ONE policy_gradient(critic) launch with a ready coefficient row
  forward    ONE advantages(critic) launch: a backward scan with two critic forwards per lane-step
  normalize  normalize_advantages(K, adv -> out, stats), one set
  torch      (A - A.mean()) / (A.std() + 1e-6)
The composed side runs kernels this change does not touch (their code objects are byte-identical to the parent's), so timing them here
is timing the parent.  Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise),
with min and max.  Every measurement runs under its own time limit."""
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
LIMIT_S = 180  # per measurement


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--normalize-only", action="store_true", help="skip the value part (sweeps of the row size for profiles/normalize.md)")
    args = ap.parse_args()
    n, K = args.n_envs, args.steps

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_value_gradient: no GPU visible (there is no CPU fallback)")
    dev, kind, d = "cuda:0", gymrs.CARTPOLE, 4
    stride = (n + 15) // 16 * 16

    def guarded(run, calls):
        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
        try:
            t0 = time.perf_counter()
            run(calls)
            return time.perf_counter() - t0
        finally:
            faulthandler.cancel_dump_traceback_later()

    def calibrate(run):
        """calls per repetition of >= 100 ms"""
        guarded(run, 1)
        c = 1
        while True:
            dt = guarded(run, c)
            if dt >= 0.1:
                return c
            c = max(c * 2, int(c * 0.1 / max(dt, 1e-6)) + 1)

    def measure(variants, label, out):
        calls = {name: calibrate(run) for name, run in variants.items()}
        times = {name: [] for name in variants}
        for _ in range(args.reps):  # taking turns
            for name, run in variants.items():
                times[name].append(guarded(run, calls[name]) / calls[name])
        for name, ts in times.items():
            out[name] = {"seconds_median": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name]}
            print(f"{label} | {name}: {np.median(ts) * 1e3:.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})", flush=True)

    result = {"gpu": torch.cuda.get_device_name(0), "n_envs": n, "steps": K, "reps": args.reps, "cases": {}}
    rand = lambda *shape: torch.randn(shape, dtype=torch.float32, device=dev)  # noqa: E731
    obs, start, returns, old_values = rand(K, d, stride), rand(d, stride), rand(K, stride), rand(K, stride)
    values, coef, adv_out = torch.zeros_like(returns), torch.zeros_like(returns), torch.zeros_like(returns)
    reward, done = torch.zeros_like(returns), torch.zeros((K, stride), dtype=torch.uint8, device=dev)
    record = dict(obs=obs.data_ptr(), actions=0, reward=reward.data_ptr(), done=done.data_ptr(), truncated=0, lane_stride=stride)
    eng = gymrs.BatchedEngine(kind, n, flags=gymrs.AUTO_RESET)
    eng.reset(seed=0)
    rng = np.random.default_rng(1)
    for hidden in () if args.normalize_only else (0, 64):
        size = gymrs.critic_size(kind, hidden)
        eng.set_critic((rng.standard_normal(size) / np.sqrt(max(hidden, d))).astype(np.float32), hidden=hidden, lanes_per_critic=n)
        grad, excl = torch.zeros((1, size), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        sums, counts = torch.zeros((1, 2), dtype=torch.int64, device=dev), torch.zeros((1, 2), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        common = dict(record=record, start_obs=start.data_ptr(), grad=grad.data_ptr(), excluded=excl.data_ptr())
        extra = dict(returns=returns.data_ptr(), values=values.data_ptr(), sums=sums.data_ptr(), counts=counts.data_ptr())

        def value(calls):
            for _ in range(calls):
                eng.value_gradient(K, old_values=old_values.data_ptr(), clip=0.2, **extra, **common)
            eng.sync()

        def plain(calls):
            for _ in range(calls):
                eng.value_gradient(K, **extra, **common)
            eng.sync()

        def forward(calls):
            for _ in range(calls):
                eng.advantages(K, record=record, start_obs=start.data_ptr(), advantages=adv_out.data_ptr(), values=values.data_ptr(), critic=True,
                               gamma=0.99, lam=0.95)
            eng.sync()

        def single(calls):
            for _ in range(calls):
                eng.policy_gradient(K, coef=coef.data_ptr(), critic=True, **common)
            eng.sync()

        def composed(calls):
            for _ in range(calls):
                torch.sub(values, returns, out=coef)
                torch.cuda.synchronize()  # the engine reads coef on its own stream
                eng.policy_gradient(K, coef=coef.data_ptr(), critic=True, **common)
                eng.advantages(K, record=record, start_obs=start.data_ptr(), advantages=adv_out.data_ptr(), values=values.data_ptr(), critic=True,
                               gamma=0.99, lam=0.95)
                eng.sync()  # torch reads values on its own stream

        out = {}
        measure({"value": value, "plain": plain, "composed": composed, "single": single, "forward": forward}, f"cartpole H={hidden}", out)
        out["value_over_composed"] = out["value"]["seconds_median"] / out["composed"]["seconds_median"]
        out["value_over_single_plus_forward"] = out["value"]["seconds_median"] / (out["single"]["seconds_median"] + out["forward"]["seconds_median"])
        out["cut_fraction"] = float(counts[0, 1]) / max(1.0, float(counts[0, 0]))
        print(f"cartpole H={hidden} | value / composed {out['value_over_composed']:.4f}, value / (single + forward) "
              f"{out['value_over_single_plus_forward']:.4f}, cut fraction {out['cut_fraction']:.3f}", flush=True)
        result["cases"][f"cartpole H={hidden}"] = out

    stats = torch.zeros(5, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def normalize(calls):
        for _ in range(calls):
            eng.normalize_advantages(K, adv=returns.data_ptr(), out=adv_out.data_ptr(), stats=stats.data_ptr(), lane_stride=stride, lanes_per_policy=n)
        eng.sync()

    def in_torch(calls):
        for _ in range(calls):
            torch.div(returns - returns.mean(), returns.std() + 1e-6, out=adv_out)
        torch.cuda.synchronize()

    out = {}
    measure({"normalize": normalize, "torch": in_torch}, "normalize", out)
    out["bytes_by_construction"] = 16 * K * n  # three reads and one write of the row
    out["normalize_bytes_per_s"] = out["bytes_by_construction"] / out["normalize"]["seconds_median"]
    out["normalize_over_torch"] = out["normalize"]["seconds_median"] / out["torch"]["seconds_median"]
    print(f"normalize | {out['normalize_bytes_per_s'] / 1e12:.3f} TB/s by construction (16 bytes per element), normalize / torch "
          f"{out['normalize_over_torch']:.4f}", flush=True)
    result["cases"]["normalize"] = out
    eng.close()
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
