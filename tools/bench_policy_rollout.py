#!/usr/bin/env python
"""Closed-loop rollouts, measured: env-steps/s of the fused policy kernel next to its ceiling (the random-policy rollout) and its
yardsticks (the per-step paths), CartPole, AUTO_RESET | TRACK_STATS.  One process; every measurement runs under its own time
limit (a stuck step dumps the stacks and ends the process).  Prints one line per figure and a JSON summary; profiles/policy_rollout.md
keeps a run.

    python tools/bench_policy_rollout.py [--n-envs 1048576] [--k 256] [--reps 9] [--commit <hash>] [--json out.json]

Each figure: median of --reps repetitions of >= 100 ms each, host clock around work that ends in a stream synchronise.
"""
from __future__ import annotations

import argparse
import faulthandler
import hashlib
import importlib
import json
import re
import shutil
import socket
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
STEP_LIMIT_S = 120  # per measurement


def kernel_source_sha16() -> str:  # as bench.kernel_source_sha16
    h = hashlib.sha256()
    for p in sorted((ROOT / "gym-rs_amd" / "csrc").glob("gymrs_*")):
        if p.suffix in (".h", ".hip"):
            h.update(p.name.encode())
            h.update(p.read_bytes())
    return h.hexdigest()[:16]


def commit_of_tree() -> str:
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def policy_kernel_resources(lib: Path) -> dict:
    """VGPR / SGPR / scratch / spill counts of the policy kernels, read from the library's code-object metadata (no GPU needed).
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
            pat = (r"\.name:\s+(\S*policy\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+)"
                   r".*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)")
            for m in re.finditer(pat, notes, re.S):
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
                name = re.sub(r"\(.*$", "", name).replace("void gymrs::", "").replace("gymrs::", "")
                out[name] = {"vgpr": int(m.group(5)), "sgpr": int(m.group(3)), "scratch_bytes": int(m.group(2)),
                             "vgpr_spill": int(m.group(6)), "sgpr_spill": int(m.group(4))}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=256, help="steps per fused launch / per step_many call")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, k = args.n_envs, args.k

    resources = policy_kernel_resources(ROOT / "gym-rs_amd" / "libgymrs_amd.so")  # before the GPU is touched

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_rollout: no GPU visible (there is no CPU fallback)")
    dev = "cuda:0"
    flags = gymrs.AUTO_RESET | gymrs.TRACK_STATS
    result = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0), "commit": args.commit or commit_of_tree(),
              "kernel_source_sha16": kernel_source_sha16(), "n_envs": n, "k": k, "reps": args.reps, "rates": {}, "rearmed_per_step": {},
              "kernel_resources": resources}

    def weights(hidden, n_policies, seed=1):  # seeded normals: scale 1 (affine), 1 / sqrt(fan_in) (hidden); not a stabilising controller
        rng = np.random.default_rng(seed)
        d, a = 4, 2
        rows = []
        for _ in range(n_policies):
            if hidden == 0:
                parts = [rng.standard_normal(a * d), rng.standard_normal(a)]
            else:
                parts = [rng.standard_normal(hidden * d) / np.sqrt(d), rng.standard_normal(hidden) / np.sqrt(d),
                         rng.standard_normal(a * hidden) / np.sqrt(hidden), rng.standard_normal(a) / np.sqrt(hidden)]
            rows.append(np.concatenate(parts).astype(np.float32))
        return np.stack(rows)

    def measure(name, eng, run, lane_steps):
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)  # this measurement's own time limit
        try:
            run(1)  # warm-up: code objects, first-touch
            eng.stats_clear()
            calls = 1
            while True:
                t0 = time.perf_counter()
                run(calls)
                dt = time.perf_counter() - t0
                if dt >= 0.1:
                    break
                calls = max(calls * 2, int(calls * 0.1 / max(dt, 1e-6)) + 1)
            rates = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                run(calls)
                rates.append(calls * lane_steps / (time.perf_counter() - t0))
            s = eng.stats()
        finally:
            faulthandler.cancel_dump_traceback_later()
        rate = float(np.median(rates))
        result["rates"][name] = rate
        result["rearmed_per_step"][name] = float(s[2] / s[3]) if s[3] else 0.0
        print(f"{name:46s} {rate:10.4g} env-steps/s   (min {min(rates):.4g}, max {max(rates):.4g}; re-armed per lane-step {s[2] / max(s[3], 1):.4f})",
              flush=True)

    def engine():
        e = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=flags)
        e.reset(seed=0)
        return e

    # the ceiling: the random-policy rollout
    eng = engine()

    def run_random(calls):
        for c in range(calls):
            eng.rollout(k, action_seed=1, action_t0=c * k)
        eng.sync()

    measure("rollout (random policy)", eng, run_random, n * k)
    eng.close()

    # the fused closed loop, weights wave-uniform (P = 1) and gathered (P = 4096, one lane per policy)
    for hidden in (0, 8, 16, 64):
        for label, n_pol, lpp in (("uniform P=1", 1, 1), ("gathered P=4096 lanes_per_policy=1", 4096, 1)):
            eng = engine()
            eng.set_policy(weights(hidden, n_pol), hidden=hidden, lanes_per_policy=lpp)

            def run_policy(calls, eng=eng):
                for _ in range(calls):
                    eng.rollout_policy(k)
                eng.sync()

            measure(f"rollout_policy H={hidden} {label}", eng, run_policy, n * k)
            eng.close()

    # the recording variant, H = 0
    eng = engine()
    eng.set_policy(weights(0, 1))
    stride = (n + 15) // 16 * 16
    k_rec = min(k, 32)  # 22 B per lane-step of trajectory: 32 steps of 2^20 lanes are 0.7 GB
    obs = torch.empty((k_rec, 4, stride), dtype=torch.float32, device=dev)
    act = torch.empty((k_rec, stride), dtype=torch.uint8, device=dev)
    rew = torch.empty((k_rec, stride), dtype=torch.float32, device=dev)
    don = torch.empty((k_rec, stride), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run_record(calls):
        for _ in range(calls):
            eng.rollout_policy_record(k_rec, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=don.data_ptr(), lane_stride=stride)
        eng.sync()

    measure(f"rollout_policy_record H=0 uniform (K={k_rec})", eng, run_record, n * k_rec)
    eng.close()
    del obs, act, rew, don

    # the per-step yardstick: actions already in 8 buffers, the policy costs nothing
    eng = engine()
    ring = torch.from_numpy(np.random.default_rng(0).integers(0, 2, (8, n)).astype(np.uint8)).to(dev)
    torch.cuda.synchronize()

    def run_step_many(calls):
        for _ in range(calls):
            eng.step_many(ring.data_ptr(), n, 8, k)
        eng.sync()

    measure("step_many (8 pre-filled action buffers)", eng, run_step_many, n * k)
    eng.close()

    # per-step closed loops: policy_actions + step, and the torch policy + step of examples/closed_loop_policy.py
    eng = engine()
    eng.set_policy(weights(0, 1))
    buf = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run_policy_actions_step(calls):
        for _ in range(calls * k):
            eng.policy_actions(buf.data_ptr())
            eng.step(buf.data_ptr())
        eng.sync()

    measure("policy_actions + step (H=0, per step)", eng, run_policy_actions_step, n * k)
    eng.close()

    class DeviceColumn:
        def __init__(self, ptr, count, typestr):
            self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 3}

    stream = torch.cuda.Stream()
    eng = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=flags)
    eng.set_stream(stream.cuda_stream)
    eng.reset(seed=0)
    x, x_dot, theta, theta_dot = (torch.as_tensor(DeviceColumn(p, n, "<f4"), device=dev) for p in eng.obs_ptrs())
    action = torch.empty(n, dtype=torch.uint8, device=dev)

    def run_torch_loop(calls):
        with torch.cuda.stream(stream):
            for _ in range(calls * k):
                torch.gt(theta + 0.5 * theta_dot + 0.05 * x_dot + 0.01 * x, 0.0, out=action.view(torch.bool))
                eng.step(action.data_ptr())
            eng.sync()

    measure("torch policy + step (examples/closed_loop_policy.py)", eng, run_torch_loop, n * k)
    eng.close()

    r = result["rates"]
    print(f"rollout_policy H=0 uniform / step_many = {r['rollout_policy H=0 uniform P=1'] / r['step_many (8 pre-filled action buffers)']:.3f}")
    if resources and "error" not in resources:
        worst = {key: max(v[key] for v in resources.values()) for key in ("vgpr", "sgpr", "scratch_bytes", "vgpr_spill", "sgpr_spill")}
        print(f"{len(resources)} policy kernels; maxima over them: {worst}")
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
