#!/usr/bin/env python
"""What softmax sampling costs inside the closed-loop fused launch: gymrs_rollout_closed_loop greedy, with GYMRS_CLOSED_LOOP_EXPLORE
at threshold 16384 and with GYMRS_CLOSED_LOOP_SAMPLE, in one process, on one engine per env and shape, taking turns
(profiles/policy_sample.md).  The yardstick is the epsilon-greedy launch.

    python tools/bench_policy_sample.py [--n-envs 1048576] [--steps 100] [--reps 9] [--json FILE]

CartPole and MountainCar, flags A | S | T, 4 lanes per work-item, K steps per call, the shapes of tools/bench_policy_explore.py
(seeded normal weights): one affine policy for every lane; 1024 affine policies in blocks of n_envs / 1024 lanes; 1024 policies with
one hidden layer of 16 units.  Variants:
  greedy    rollout_closed_loop(K): the argmax
  epsilon   rollout_closed_loop(K, explore) at threshold 16384 (epsilon 0.25)
  sample    rollout_closed_loop(K, sample) at temperature 1
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a stream synchronise), with min and
max; the variants take turns repetition by repetition, so drift of the clocks meets all three alike.  Also prints registers, scratch
and spills of the sampling kernel families from the library's code-object metadata (no GPU needed for that part:
--resources-only).  Every measurement runs under its own time limit."""
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
THRESHOLD = 16384

from bench_policy_rollout import kernel_source_sha16  # noqa: E402


def sample_kernel_resources(lib: Path) -> dict:
    """VGPR / SGPR / scratch / spill counts of the sampling kernels, read from the library's code-object metadata.  Called before the
    HIP runtime is up: it starts child processes."""
    llvm = next((d for d in (Path("/opt/rocm/llvm/bin"), Path(shutil.which("llvm-readelf") or "/nonexistent").parent) if (d / "llvm-readelf").exists()), None)
    if llvm is None:
        return {"error": "llvm-readelf not found"}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, Path(tmp) / "lib.so")
        subprocess.run([str(llvm / "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        for co in sorted(Path(tmp).glob("lib.so.*amdgcn*")):
            notes = subprocess.run([str(llvm / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
            pat = (r"\.name:\s+(\S*sample\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+)"
                   r".*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)")
            found = list(re.finditer(pat, notes, re.S))
            names = subprocess.run(["c++filt"], input="\n".join(m.group(1) for m in found), capture_output=True, text=True).stdout.split("\n")
            for m, name in zip(found, names):
                name = re.sub(r"\(.*$", "", name.strip() or m.group(1)).replace("void gymrs::", "").replace("gymrs::", "")
                out[name] = {"vgpr": int(m.group(5)), "sgpr": int(m.group(3)), "scratch_bytes": int(m.group(2)),
                             "vgpr_spill": int(m.group(6)), "sgpr_spill": int(m.group(4))}
    return out


def families(resources: dict) -> dict:
    """The sampling kernels grouped per family (kernel, env type, lanes per work-item, recording): ranges over the flag sets, and
    which flag sets use scratch (flag set, bytes, VGPRs spilled)"""
    out = {}
    fields = ("vgpr", "sgpr", "scratch_bytes", "vgpr_spill", "sgpr_spill")
    for name, v in resources.items():
        m = re.match(r"(rollout_sample(?:_fitness|_transitions)?_kernel)<(TableT<\w+>|\w+), (?:(\d+), )?(\d+)u(?:, (true|false))?>", name)
        if not m or not isinstance(v, dict):
            continue
        key = f"{m.group(1)}<{m.group(2)}, {m.group(3) or 4}{', recording' if m.group(5) == 'true' else ''}>"
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
    ap.add_argument("--resources-only", action="store_true", help="print the kernel families' registers and scratch and stop (no GPU)")
    args = ap.parse_args()
    n, K = args.n_envs, args.steps
    lib_path = importlib.import_module("gym-rs_amd._lib").library_path()
    resources = sample_kernel_resources(lib_path)  # before the GPU is touched
    fams = families(resources)
    if args.resources_only:
        for name in sorted(fams):
            print(name, fams[name])
        for name in sorted(k for k in resources if k.startswith("sample_actions_kernel")):
            print(name, resources[name])
        return 0

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_sample: no GPU visible (there is no CPU fallback)")
    flags = gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT
    shapes = (("uniform affine", 1, 0), ("1024 affine", 1024, 0), ("1024 x H16", 1024, 16))
    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "library": str(lib_path.name), "n_envs": n,
              "steps": K, "flags": flags, "reps": args.reps, "threshold": THRESHOLD, "temperature": 1.0, "envs": {}, "kernel_families": fams,
              "sample_actions_kernels": {k: v for k, v in resources.items() if k.startswith("sample_actions_kernel")}}
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
            eng.set_exploration(7, threshold=THRESHOLD)
            eng.set_sampling(7, temperature=1.0)

            def launch(**kw):
                def run(calls):
                    for _ in range(calls):
                        eng.rollout_closed_loop(K, **kw)
                    eng.sync()
                return run

            variants = {"greedy": launch(), "epsilon": launch(explore=True), "sample": launch(sample=True)}
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
            out["sample_over_epsilon"] = out["sample"]["seconds_median"] / out["epsilon"]["seconds_median"]
            out["sample_over_greedy"] = out["sample"]["seconds_median"] / out["greedy"]["seconds_median"]
            result["envs"][env][shape] = out
            for name in variants:
                v = out[name]
                print(f"{env} | {shape} | {name}: {K} steps {v['seconds_median'] * 1e3:.3f} ms (min {v['seconds_min'] * 1e3:.3f}, max "
                      f"{v['seconds_max'] * 1e3:.3f}), {v['lane_steps_per_s']:.4g} lane-steps/s", flush=True)
            print(f"{env} | {shape} | sample / epsilon {out['sample_over_epsilon']:.3f}, sample / greedy {out['sample_over_greedy']:.3f}", flush=True)
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
