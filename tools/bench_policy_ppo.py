#!/usr/bin/env python
"""One PPO epoch over a record: gymrs_ppo_gradient against the two gymrs_policy_gradient launches it replaces
(profiles/policy_ppo.md).  One process, taking turns:

    python tools/bench_policy_ppo.py [--n-envs 1048576] [--steps 64] [--reps 5] [--json FILE] [--resources-only]

CartPole with H = 0, 16 and 64 and MountainCar with H = 0 (one policy for all lanes), temperature 1, clip 0.2, a record written by
rollout_transitions(sample=True) on an engine with A | S | T, advantages drawn once (standard normal), old_prob = the prob row of
weights a small step away from the ones the epoch runs under (so that some lane-steps are cut).
  (a) fused      ppo_gradient(K, record, start_obs, advantages, old_prob -> grad, excluded, counts): ONE launch
  (b) composed   what a user has without it: policy_gradient for the prob row (its gradient is thrown away), a synchronise, the
                 coefficient row in torch (ratio, the two compares, where), a synchronise, policy_gradient with that row
  (c) launches   the two policy_gradient launches of (b) alone, back to back
  (d) single     ONE policy_gradient launch with a prob row: what the fused call costs beyond it is the price of the feature
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max.
Also checks that (a) and (b) leave the same table, reports the clip fraction, the bytes moved by construction per lane-step for the
affine networks, and the registers and scratch of every gradient kernel from the library's code-object metadata (`--resources-only`:
nothing else, no GPU).  Every measurement runs under its own time limit."""
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
LIMIT_S = 180  # per measurement

from bench_policy_gradient import kernel_resources  # noqa: E402  (matches gradient_kernel and gradient_ppo_kernel alike)
from bench_policy_rollout import kernel_source_sha16  # noqa: E402


def bytes_per_lane_step(d: int, fused: bool) -> int:
    """by construction, affine networks: one read of the observation, the coefficient (advantage) row and the action; the fused call
    reads the old-probability row as well"""
    return 4 * d + 4 + 1 + (4 if fused else 0)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    n, K = args.n_envs, args.steps
    lib_path = importlib.import_module("gym-rs_amd._lib").library_path()
    resources = kernel_resources(lib_path)  # before the GPU is touched
    if args.resources_only:
        for name in sorted(resources):
            print(name, resources[name])
        return 0

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_ppo: no GPU visible (there is no CPU fallback)")
    dev = "cuda:0"
    A_S_T = gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT
    low, high = float(np.float32(1 - 0.2)), float(np.float32(1 + 0.2))

    def calibrate(run):
        """calls per repetition of >= 100 ms"""
        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
        try:
            run(1)
            c = 1
            while True:
                t0 = time.perf_counter()
                run(c)
                dt = time.perf_counter() - t0
                if dt >= 0.1:
                    break
                c = max(c * 2, int(c * 0.1 / max(dt, 1e-6)) + 1)
        finally:
            faulthandler.cancel_dump_traceback_later()
        return c

    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "library": str(lib_path.name), "n_envs": n, "steps": K,
              "reps": args.reps, "clip": [low, high], "cases": {}, "kernels": resources}
    stride = (n + 15) // 16 * 16
    scale = 1.4426950408889634
    for env, kind, hiddens in (("cartpole", gymrs.CARTPOLE, (0, 16, 64)), ("mountain_car", gymrs.MOUNTAIN_CAR, (0,))):
        d = 4 if kind == gymrs.CARTPOLE else 2
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        obs, final, start, rew = f32(K, d, stride), f32(K, d, stride), f32(d, stride), f32(K, stride)
        act, done, trunc = u8(K, stride), u8(K, stride), u8(K, stride)
        adv = torch.randn((K, stride), dtype=torch.float32, device=dev)
        old_prob, prob, coef = f32(K, stride), f32(K, stride), f32(K, stride)
        torch.cuda.synchronize()
        record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                      lane_stride=stride)
        rng = np.random.default_rng(1)
        eng = gymrs.BatchedEngine(kind, n, flags=A_S_T)
        eng.reset(seed=0)
        for hidden in hiddens:
            size = gymrs.policy_size(kind, hidden)
            w_old = (rng.standard_normal(size) / np.sqrt(max(hidden, d))).astype(np.float32)
            w_new = (w_old + 0.5 * rng.standard_normal(size) / np.sqrt(max(hidden, d))).astype(np.float32)
            grad = torch.zeros((1, size), dtype=torch.int64, device=dev)
            excl = torch.zeros(1, dtype=torch.int64, device=dev)
            counts = torch.zeros((1, 2), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            eng.set_policy(w_old, hidden=hidden, lanes_per_policy=n)
            eng.set_sampling(7, temperature=1.0)
            eng.rollout_transitions(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), sample=True)
            common = dict(record=record, start_obs=start.data_ptr(), grad=grad.data_ptr(), excluded=excl.data_ptr(), scale=scale)
            eng.policy_gradient(K, coef=adv.data_ptr(), prob=old_prob.data_ptr(), **common)  # old_prob: the record's own probabilities
            eng.sync()
            eng.set_policy(w_new, hidden=hidden, lanes_per_policy=n)  # the epoch runs under the moved weights
            eng.sync()

            def fused(calls):
                for _ in range(calls):
                    eng.ppo_gradient(K, advantages=adv.data_ptr(), old_prob=old_prob.data_ptr(), counts=counts.data_ptr(), clip_low=low, clip_high=high, **common)
                eng.sync()

            def composed(calls):
                for _ in range(calls):
                    eng.policy_gradient(K, coef=adv.data_ptr(), prob=prob.data_ptr(), **common)
                    eng.sync()  # torch reads prob on its own stream
                    ratio = prob / old_prob
                    cut = ((adv > 0) & (ratio > high)) | ((adv < 0) & (ratio < low))
                    torch.where(cut, torch.zeros_like(adv), adv * ratio, out=coef)
                    torch.cuda.synchronize()  # the engine reads coef on its own stream
                    eng.policy_gradient(K, coef=coef.data_ptr(), **common)
                eng.sync()

            def launches(calls):
                for _ in range(calls):
                    eng.policy_gradient(K, coef=adv.data_ptr(), prob=prob.data_ptr(), **common)
                    eng.policy_gradient(K, coef=coef.data_ptr(), **common)
                eng.sync()

            def single(calls):
                for _ in range(calls):
                    eng.policy_gradient(K, coef=adv.data_ptr(), prob=prob.data_ptr(), **common)
                eng.sync()

            # the same table from (a) and (b), once, before the timing
            def table_of(run):
                grad.zero_()
                excl.zero_()
                counts.zero_()
                torch.cuda.synchronize()
                run()
                eng.sync()
                return grad.clone(), int(excl[0])

            g_fused, x_fused = table_of(lambda: eng.ppo_gradient(K, advantages=adv.data_ptr(), old_prob=old_prob.data_ptr(), counts=counts.data_ptr(),
                                                                 clip_low=low, clip_high=high, **common))
            seen, cut = (int(v) for v in counts[0])
            composed(1)  # leaves the coefficient row in coef
            g_comp, x_comp = table_of(lambda: eng.policy_gradient(K, coef=coef.data_ptr(), **common))
            same = bool(torch.equal(g_fused, g_comp)) and x_fused == x_comp

            variants = {"fused": fused, "composed": composed, "launches": launches, "single": single}
            label = f"{env} H={hidden}"
            calls = {name: calibrate(run) for name, run in variants.items()}
            times = {name: [] for name in variants}
            for _ in range(args.reps):  # taking turns
                for name, run in variants.items():
                    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
                    try:
                        t0 = time.perf_counter()
                        run(calls[name])
                        times[name].append((time.perf_counter() - t0) / calls[name])
                    finally:
                        faulthandler.cancel_dump_traceback_later()
            out = {"same_table_as_composed": same, "excluded": x_fused, "lane_steps": seen, "cut": cut, "clip_fraction": cut / max(1, seen)}
            for name in variants:
                ts = times[name]
                med = float(np.median(ts))
                out[name] = {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name]}
                print(f"{label} | {name}: {med * 1e3:.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})", flush=True)
            out["fused_below_launches_ranges_apart"] = out["fused"]["seconds_max"] < out["launches"]["seconds_min"]
            out["fused_over_composed"] = out["fused"]["seconds_median"] / out["composed"]["seconds_median"]
            out["fused_over_launches"] = out["fused"]["seconds_median"] / out["launches"]["seconds_median"]
            out["fused_over_single"] = out["fused"]["seconds_median"] / out["single"]["seconds_median"]
            if hidden == 0:
                out["bytes_per_lane_step"] = {"fused": bytes_per_lane_step(d, True), "single": bytes_per_lane_step(d, False) + 4}  # single writes prob
                out["fused_bytes_per_s"] = bytes_per_lane_step(d, True) * n * K / out["fused"]["seconds_median"]
            print(f"{label} | fused / composed {out['fused_over_composed']:.4f}, fused / launches {out['fused_over_launches']:.4f} (ranges apart: "
                  f"{out['fused_below_launches_ranges_apart']}), fused / single {out['fused_over_single']:.4f}; same table {same}; cut {cut} of {seen} "
                  f"({out['clip_fraction']:.3f}); excluded {x_fused}", flush=True)
            result["cases"][label] = out
            torch.cuda.empty_cache()
        eng.close()
        del obs, final, start, rew, act, done, trunc, adv, old_prob, prob, coef
        torch.cuda.empty_cache()
    for name in sorted(resources):
        print(name, resources[name])
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
