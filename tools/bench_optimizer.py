#!/usr/bin/env python
"""gymrs_apply_gradient against the bytes it moves and against the torch update it replaces (profiles/optimizer.md).  One process:

    python tools/bench_optimizer.py [--hidden 16] [--reps 5] [--json FILE]

CartPole policies with H = 16 (S = 114), n_sets = 1, 2^12 and 2^16, one lane per set.
  apply   apply_gradient(adam=True, max_norm=1, zero_grad=True, skipped=...) on the policy head: ONE launch per call, no
          synchronisation between calls.  It moves 40 B per parameter by construction (q read and zeroed 16, w 8, m 8, v 8); the
          first call of a window reads the random table, the later ones the zeros it left (the kernel's work does not depend on the
          values).
  torch   the update of examples/ppo_cartpole.py on the same table, in the engine's weights through policy_weights_ptr:
          w += (lr * g.double() * 2**-24 / N).float(), g.zero_(), x.zero_(), and the torch.cuda.synchronize() that hands the tables
          back to the engine's stream.  Plain SGD: no moments, no clip, excluded not looked at.
  copy    a 1 GiB device copy (read + write): the bandwidth yardstick of the other profiles.
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max,
taking turns.  Every measurement runs under its own time limit."""
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
BYTES_PER_PARAM = 40  # q read + zeroed, w, m, v read + written


class DeviceFloats:
    """n floats at a device address, for torch.as_tensor (zero-copy)"""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer: no GPU visible (there is no CPU fallback)")
    dev = "cuda:0"

    def timed(run, calls):
        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
        try:
            t0 = time.perf_counter()
            run(calls)
            return time.perf_counter() - t0
        finally:
            faulthandler.cancel_dump_traceback_later()

    def calibrate(run):
        """calls per repetition of >= 100 ms"""
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

    src, dst = torch.empty(1 << 28, dtype=torch.float32, device=dev), torch.empty(1 << 28, dtype=torch.float32, device=dev)

    def copy(calls):
        for _ in range(calls):
            dst.copy_(src)
        torch.cuda.synchronize()

    copy_rate = 2 * (1 << 30) / measure({"copy": copy})["copy"]["seconds_median"]
    del src, dst
    torch.cuda.empty_cache()
    print(f"copy yardstick: {copy_rate / 1e12:.3f} TB/s (1 GiB device copy, read + write)", flush=True)

    kind, hidden = gymrs.CARTPOLE, args.hidden
    size = gymrs.policy_size(kind, hidden)
    rng = np.random.default_rng(1)
    result = {"gpu": torch.cuda.get_device_name(0), "hidden": hidden, "params_per_set": size, "reps": args.reps, "copy_bytes_per_s": copy_rate,
              "bytes_per_param": BYTES_PER_PARAM, "cases": {}}
    for n_sets in (1, 1 << 12, 1 << 16):
        eng = gymrs.BatchedEngine(kind, 1024, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT)
        eng.reset(seed=0)
        eng.set_policy((0.1 * rng.standard_normal((n_sets, size))).astype(np.float32), hidden=hidden, lanes_per_policy=1)
        grad = torch.randint(-(1 << 40), 1 << 40, (n_sets, size), dtype=torch.int64, device=dev)
        excluded, skipped = torch.zeros(n_sets, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        table = torch.as_tensor(DeviceFloats(*eng.policy_weights_ptr()), device=dev).view(n_sets, size)
        torch.cuda.synchronize()

        def apply(calls):
            for _ in range(calls):
                eng.apply_gradient(grad=grad.data_ptr(), excluded=excluded.data_ptr(), skipped=skipped.data_ptr(), adam=True, lr=1e-3,
                                   grad_scale=2.0**-24 / 4096, max_norm=1.0, ascend=True, zero_grad=True)
            eng.sync()

        def torch_update(calls):
            for _ in range(calls):
                table.add_((1e-3 * grad.double() * 2.0**-24 / 4096).float())
                grad.zero_()
                excluded.zero_()
                torch.cuda.synchronize()  # the engine's next launch reads on its own stream

        out = measure({"apply": apply, "torch": torch_update})
        moved = n_sets * size * BYTES_PER_PARAM
        out["bytes_moved"] = moved
        out["apply_bytes_per_s"] = moved / out["apply"]["seconds_median"]
        out["apply_share_of_copy"] = out["apply_bytes_per_s"] / copy_rate
        out["torch_over_apply"] = out["torch"]["seconds_median"] / out["apply"]["seconds_median"]
        for name in ("apply", "torch"):
            t = out[name]
            print(f"n_sets={n_sets} | {name}: {t['seconds_median'] * 1e6:.2f} us (min {t['seconds_min'] * 1e6:.2f}, max {t['seconds_max'] * 1e6:.2f})", flush=True)
        print(f"n_sets={n_sets} | apply moves {moved / 1e6:.3f} MB: {out['apply_bytes_per_s'] / 1e12:.3f} TB/s, {out['apply_share_of_copy']:.2f} of the copy; "
              f"torch / apply = {out['torch_over_apply']:.1f}", flush=True)
        result["cases"][f"n_sets={n_sets}"] = out
        eng.close()
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
