#!/usr/bin/env python
"""What epsilon-greedy exploration costs inside the closed-loop fused launch, and what the fused launch buys over the per-step loop
it replaces: gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_EXPLORE at three thresholds against three yardsticks, in one process,
on one engine per env and shape, taking turns (profiles/policy_explore.md).

    python tools/bench_policy_explore.py [--n-envs 1048576] [--steps 100] [--reps 9] [--json FILE]

CartPole and MountainCar, flags A | S | T, 4 lanes per work-item, K steps per call.  Shapes (seeded normal weights):
  uniform affine       one affine policy for every lane
  1024 affine          1024 affine policies, lanes_per_policy = n_envs / 1024 (every wave uniform in its policy)
  1024 x H16           1024 policies with one hidden layer of 16 units, same blocks
Variants:
  explore 0 / 6554 / 65536   rollout_closed_loop(K, explore) at that threshold (epsilon 0, 0.1, 1): ONE launch
  greedy                     gymrs_rollout_policy(K): the greedy fused launch
  random                     gymrs_rollout(K): the random-policy fused launch (explores, ignores the state)
  loop                       K x (gymrs_explore_actions + gymrs_step) at threshold 6554: 2K launches, what a caller had to write
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a stream synchronise), with min and
max; the variants take turns repetition by repetition.  Also prints registers, scratch, spills and waves per SIMD of the exploring
kernel families from the library's code-object metadata.  Every measurement runs under its own time limit."""
from __future__ import annotations

import argparse
import faulthandler
import importlib
import json
import re
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
LIMIT_S = 120  # per measurement
THRESHOLDS = (0, 6554, 65536)

from bench_policy_rollout import kernel_source_sha16  # noqa: E402


def explore_kernel_resources(lib: Path) -> dict:
    """VGPR / SGPR / scratch / spill counts of the exploring kernels, read from the library's code-object metadata (no GPU needed).
    Called before the HIP runtime is up: it starts child processes."""
    llvm = next((d for d in (Path("/opt/rocm/llvm/bin"), Path(shutil.which("llvm-readelf") or "/nonexistent").parent) if (d / "llvm-readelf").exists()), None)
    if llvm is None:
        return {"error": "llvm-readelf not found"}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, Path(tmp) / "lib.so")
        subprocess.run([str(llvm / "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        for co in sorted(Path(tmp).glob("lib.so.*amdgcn*")):
            notes = subprocess.run([str(llvm / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
            pat = (r"\.name:\s+(\S*explore\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+)"
                   r".*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)")
            for m in re.finditer(pat, notes, re.S):
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
                name = re.sub(r"\(.*$", "", name).replace("void gymrs::", "").replace("gymrs::", "")
                out[name] = {"vgpr": int(m.group(5)), "sgpr": int(m.group(3)), "scratch_bytes": int(m.group(2)),
                             "vgpr_spill": int(m.group(6)), "sgpr_spill": int(m.group(4))}
    return out


def families(resources: dict) -> dict:
    """The exploring kernels grouped per family (kernel, env type, lanes per work-item, recording): ranges over the ten flag sets, and
    which flag sets use scratch (flag set, bytes, VGPRs spilled)"""
    out = {}
    fields = ("vgpr", "sgpr", "scratch_bytes", "vgpr_spill", "sgpr_spill")
    for name, v in resources.items():
        m = re.match(r"(rollout_explore(?:_fitness)?_kernel)<(TableT<\w+>|\w+), (\d+), (\d+)u(?:, (true|false))?>", name)
        if not m or not isinstance(v, dict):
            continue
        key = f"{m.group(1)}<{m.group(2)}, {m.group(3)}{', recording' if m.group(5) == 'true' else ''}>"
        f = out.setdefault(key, {"kernels": 0, "scratch_at": [], **{k: [] for k in fields}})
        f["kernels"] += 1
        for k in fields:
            f[k].append(v[k])
        if v["scratch_bytes"]:
            f["scratch_at"].append([int(m.group(4)), v["scratch_bytes"], v["vgpr_spill"]])
    for f in out.values():
        for k in fields:
            f[k] = [min(f[k]), max(f[k])]
        f["scratch_at"].sort()
        f["waves_per_simd"] = min(8, 512 // max(8, (f["vgpr"][1] + 7) // 8 * 8))  # the 512 VGPRs of a gfx950 SIMD, allocation granule 8
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, K = args.n_envs, args.steps
    lib_path = importlib.import_module("gym-rs_amd._lib").library_path()
    resources = explore_kernel_resources(lib_path)  # before the GPU is touched
    fams = families(resources)

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_explore: no GPU visible (there is no CPU fallback)")
    flags = gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT
    shapes = (("uniform affine", 1, 0), ("1024 affine", 1024, 0), ("1024 x H16", 1024, 16))
    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "library": str(lib_path.name), "n_envs": n,
              "steps": K, "flags": flags, "reps": args.reps, "thresholds": list(THRESHOLDS), "envs": {}, "kernel_families": fams,
              "explore_actions_kernels": {k: v for k, v in resources.items() if k.startswith("explore_actions_kernel")}}
    for env, kind in (("cartpole", gymrs.CARTPOLE), ("mountain_car", gymrs.MOUNTAIN_CAR)):
        result["envs"][env] = {}
        for shape, n_policies, hidden in shapes:
            rng = np.random.default_rng(1)
            size = gymrs.policy_size(kind, hidden)
            scale = 1.0 if hidden == 0 else 0.5
            weights = (rng.standard_normal((n_policies, size)) * scale).astype(np.float32)
            eng = gymrs.BatchedEngine(kind, n, flags=flags)
            eng.reset(seed=0)
            eng.set_policy(weights, hidden=hidden, lanes_per_policy=max(1, n // n_policies))
            act = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()

            def explore(threshold):
                def run(calls):
                    eng.set_exploration(7, threshold=threshold)
                    for _ in range(calls):
                        eng.rollout_closed_loop(K, explore=True)
                    eng.sync()
                return run

            def greedy(calls):
                for _ in range(calls):
                    eng.rollout_policy(K)
                eng.sync()

            def random_policy(calls):
                for c in range(calls):
                    eng.rollout(K, 11, c * K)
                eng.sync()

            def loop(calls):
                eng.set_exploration(7, threshold=6554)
                for _ in range(calls * K):
                    eng.explore_actions(act.data_ptr())
                    eng.step(act.data_ptr())
                eng.sync()

            variants = {f"explore {t}": explore(t) for t in THRESHOLDS}
            variants.update({"greedy": greedy, "random": random_policy, "loop": loop})
            calls, times = {}, {name: [] for name in variants}
            faulthandler.dump_traceback_later(LIMIT_S, exit=True)
            try:
                for name, run in variants.items():  # warm-up, and how many calls make 100 ms
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
                for name, run in variants.items():
                    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
                    try:
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
            for t in THRESHOLDS:
                out[f"explore {t}"]["over_loop"] = out[f"explore {t}"]["seconds_median"] / out["loop"]["seconds_median"]
                out[f"explore {t}"]["over_greedy"] = out[f"explore {t}"]["seconds_median"] / out["greedy"]["seconds_median"]
            out["fused_beats_loop"] = all(out[f"explore {t}"]["seconds_median"] < out["loop"]["seconds_median"] for t in THRESHOLDS)
            result["envs"][env][shape] = out
            for name in variants:
                v = out[name]
                print(f"{env} | {shape} | {name}: {K} steps {v['seconds_median'] * 1e3:.3f} ms (min {v['seconds_min'] * 1e3:.3f}, max "
                      f"{v['seconds_max'] * 1e3:.3f}), {v['lane_steps_per_s']:.4g} lane-steps/s"
                      + (f", / loop {v['over_loop']:.3f}, / greedy {v['over_greedy']:.3f}" if "over_loop" in v else ""), flush=True)
    for name in sorted(fams):
        print(name, fams[name])
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    ok = all(shape["fused_beats_loop"] for env in result["envs"].values() for shape in env.values())
    print("the fused exploring launch beats the loop at every shape measured" if ok else "THE LOOP WON SOMEWHERE: see fused_beats_loop")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
