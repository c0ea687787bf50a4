#!/usr/bin/env python
"""gymrs_q_gradient beside gymrs_policy_gradient on the same record (profiles/q_gradient.md).  One process, taking turns:

    python tools/bench_q_gradient.py [--n-envs 1048576] [--steps 64] [--reps 5] [--json FILE]

CartPole with H = 0 and 64 (one policy for all lanes), a record written by rollout_transitions(explore=True, epsilon 0.1) on an engine
with A | S | T, gamma 0.99, kappa 1, a target set one small step away from the online set.
  q plain / q double   q_gradient(K, record, start_obs, final_obs -> td, grad, excluded, counts): TWO kernels (q_td_kernel, then
                       q_gradient_kernel), without and with GYMRS_Q_DOUBLE
  policy               ONE policy_gradient launch over the same rows with a coefficient row (no prob row)
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max.
The host clock sees the call, not its kernels: run the tool under a kernel trace (rocprofv3 --kernel-trace --stats -- python ...) for
the time of each of the two.  Every measurement runs under its own time limit."""
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


def bytes_per_lane_step(d: int) -> dict:
    """by construction, affine networks.  TD kernel: one read of obs, reward, done, truncated and the action, one write of td;
    gradient kernel: obs, the action and td again.  A fused kernel would read each row once and write td."""
    td = 4 * d + 4 + 1 + 1 + 1 + 4
    return {"td_kernel": td, "gradient_kernel": 4 * d + 1 + 4, "both": td + 4 * d + 1 + 4, "fused_by_construction": td}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, K = args.n_envs, args.steps

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_q_gradient: no GPU visible (there is no CPU fallback)")
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

    kind, d = gymrs.CARTPOLE, 4
    stride = (n + 15) // 16 * 16
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    obs, final, start, rew, td = f32(K, d, stride), f32(K, d, stride), f32(d, stride), f32(K, stride), f32(K, stride)
    act, done, trunc = u8(K, stride), u8(K, stride), u8(K, stride)
    coef = torch.randn((K, stride), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(), lane_stride=stride)
    rng = np.random.default_rng(1)
    eng = gymrs.BatchedEngine(kind, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT)
    eng.reset(seed=0)
    eng.set_exploration(7, epsilon=0.1)
    result = {"gpu": torch.cuda.get_device_name(0), "n_envs": n, "steps": K, "reps": args.reps, "bytes_per_lane_step": bytes_per_lane_step(d), "cases": {}}
    for hidden in (0, 64):
        size = gymrs.policy_size(kind, hidden)
        w = (rng.standard_normal(size) / np.sqrt(max(hidden, d))).astype(np.float32)
        tables = [torch.zeros(shape, dtype=torch.int64, device=dev) for shape in ((1, size), (1,), (1, 2))]
        torch.cuda.synchronize()
        eng.set_policy((w + 0.1 * rng.standard_normal(size) / np.sqrt(max(hidden, d))).astype(np.float32), hidden=hidden, lanes_per_policy=n)
        eng.q_target_sync()
        eng.set_policy(w, hidden=hidden, lanes_per_policy=n)
        eng.rollout_transitions(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), explore=True)
        eng.sync()
        common = dict(record=record, start_obs=start.data_ptr(), grad=tables[0].data_ptr(), excluded=tables[1].data_ptr())

        def q(double):
            def run(calls):
                for _ in range(calls):
                    eng.q_gradient(K, final_obs=final.data_ptr(), td=td.data_ptr(), counts=tables[2].data_ptr(), gamma=0.99, kappa=1.0, double=double, **common)
                eng.sync()
            return run

        def policy(calls):
            for _ in range(calls):
                eng.policy_gradient(K, coef=coef.data_ptr(), temperature=1.0, **common)
            eng.sync()

        variants = {"q plain": q(False), "q double": q(True), "policy": policy}
        calls = {name: calibrate(run) for name, run in variants.items()}
        times = {name: [] for name in variants}
        for _ in range(args.reps):  # taking turns
            for name, run in variants.items():
                times[name].append(timed(run, calls[name]) / calls[name])
        seen, clamped = (int(v) for v in tables[2][0])
        out = {"lane_steps_seen": seen, "clamped_fraction": clamped / max(1, seen), "ended_fraction": float(((done != 0) | (trunc != 0)).float().mean())}
        for name, ts in times.items():
            out[name] = {"seconds_median": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name]}
            print(f"cartpole H={hidden} | {name}: {np.median(ts) * 1e3:.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})", flush=True)
        result["cases"][f"cartpole H={hidden}"] = out
    eng.close()
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
