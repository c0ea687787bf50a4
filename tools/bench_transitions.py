#!/usr/bin/env python
"""What per-step final observations cost inside the recorded closed-loop launch, and what the launch buys over the only other
correct way to collect whole transitions (profiles/transitions.md).  One process, one engine per env and table setting, the
variants taking turns:

    python tools/bench_transitions.py [--n-envs 1048576] [--steps 100] [--reps 9] [--json FILE]

CartPole and MountainCar, flags A | S | T, one affine policy, K steps per call, without and with a five-row parameter table.
  (a) record        rollout_closed_loop(K, record): today's recorded launch (final observations of all but a lane's last ending lost)
  (b) transitions   rollout_transitions(K, record, final_obs, start_obs): ONE launch, whole transitions
  (b0) explore 0    (a) with GYMRS_CLOSED_LOOP_EXPLORE at threshold 0: the exploring action source playing greedy, which is the source
                    (b) uses for greedy launches -- (b0) / (a) is what sharing one source costs
  (c) loop          K x (policy_actions + step) on an engine with GYMRS_FINAL_OBS, with a device copy of the final-observation arrays
                    after every step on the engine's stream: the alternative that was correct before (it keeps no record rows, so it
                    is charged less than it would need)
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a stream synchronise), with min and
max.  Also reports the ended share of lane-steps of a recorded launch (what the extra stores scale with) and the registers, scratch
and spills of the transition kernels from the library's code-object metadata.  Every measurement runs under its own time limit."""
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

from bench_policy_rollout import kernel_source_sha16  # noqa: E402


def kernel_resources(lib: Path) -> dict:
    """VGPR / SGPR / scratch / spill counts of rollout_transitions_kernel<..>, from the code-object metadata (no GPU needed).  Called
    before the HIP runtime is up: it starts child processes."""
    llvm = next((d for d in (Path("/opt/rocm/llvm/bin"), Path(shutil.which("llvm-readelf") or "/nonexistent").parent) if (d / "llvm-readelf").exists()), None)
    if llvm is None:
        return {"error": "llvm-readelf not found"}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, Path(tmp) / "lib.so")
        subprocess.run([str(llvm / "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True, stdin=subprocess.DEVNULL)
        for co in sorted(Path(tmp).glob("lib.so.*amdgcn*")):
            notes = subprocess.run([str(llvm / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout
            pat = (r"\.name:\s+(\S*rollout_transitions\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+)"
                   r".*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)")
            for m in re.finditer(pat, notes, re.S):
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout.strip() or m.group(1)
                name = re.sub(r"\(.*$", "", name).replace("void gymrs::", "").replace("gymrs::", "")
                out[name] = {"vgpr": int(m.group(5)), "sgpr": int(m.group(3)), "scratch_bytes": int(m.group(2)),
                             "vgpr_spill": int(m.group(6)), "sgpr_spill": int(m.group(4))}
    return out


class View:
    """A zero-copy torch view of a device array"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, K = args.n_envs, args.steps
    lib_path = importlib.import_module("gym-rs_amd._lib").library_path()
    resources = kernel_resources(lib_path)  # before the GPU is touched

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_transitions: no GPU visible (there is no CPU fallback)")
    A_S_T = gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT
    scaled = {gymrs.CARTPOLE: ("length", "masspole", "force_mag", "gravity"), gymrs.MOUNTAIN_CAR: ("force", "gravity")}
    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "n_envs": n, "steps": K, "flags": A_S_T,
              "reps": args.reps, "envs": {}, "kernels": resources}
    stride = (n + 15) // 16 * 16
    for env, kind in (("cartpole", gymrs.CARTPOLE), ("mountain_car", gymrs.MOUNTAIN_CAR)):
        d = 4 if kind == gymrs.CARTPOLE else 2
        obs = torch.empty((K, d, stride), dtype=torch.float32, device="cuda:0")
        final = torch.empty((K, d, stride), dtype=torch.float32, device="cuda:0")
        start = torch.empty((d, stride), dtype=torch.float32, device="cuda:0")
        act = torch.empty((K, stride), dtype=torch.uint8, device="cuda:0")
        rew = torch.empty((K, stride), dtype=torch.float32, device="cuda:0")
        done = torch.empty((K, stride), dtype=torch.uint8, device="cuda:0")
        trunc = torch.empty((K, stride), dtype=torch.uint8, device="cuda:0")
        buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                      lane_stride=stride)
        result["envs"][env] = {}
        for table in (False, True):
            rng = np.random.default_rng(1)
            weights = rng.standard_normal((1, gymrs.policy_size(kind, 0))).astype(np.float32)
            base = gymrs.engine.default_params(kind)
            engines = []
            for flags in (A_S_T, A_S_T | gymrs.FINAL_OBS):
                eng = gymrs.BatchedEngine(kind, n, flags=flags, params=base)
                if table:
                    rows = []
                    for _ in range(5):
                        p = type(base).from_buffer_copy(base)
                        for f in scaled[kind]:
                            setattr(p, f, getattr(p, f) * float(rng.uniform(0.5, 1.5)))
                        rows.append(p)
                    eng.set_param_table(rows)
                    eng.set_param_index(rng.integers(0, 5, n).astype(np.uint16))
                eng.reset(seed=0)
                eng.set_policy(weights, hidden=0, lanes_per_policy=n)
                eng.set_exploration(7, threshold=0)
                engines.append(eng)
            eng, per_step = engines
            views = [torch.as_tensor(View(p, n), device="cuda:0") for p in per_step.final_obs_ptrs()]
            on_stream = torch.cuda.ExternalStream(per_step.stream) if per_step.stream else torch.cuda.default_stream()

            def rec(calls):
                for _ in range(calls):
                    eng.rollout_closed_loop(K, lane_params=table, record=record)
                eng.sync()

            def rec0(calls):
                for _ in range(calls):
                    eng.rollout_closed_loop(K, lane_params=table, record=record, explore=True)
                eng.sync()

            def trans(calls):
                for _ in range(calls):
                    eng.rollout_transitions(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), lane_params=table)
                eng.sync()

            def loop(calls):
                with torch.cuda.stream(on_stream):
                    for _ in range(calls):
                        for k in range(K):
                            per_step.policy_actions(buf.data_ptr())
                            per_step.step(buf.data_ptr())
                            for j, v in enumerate(views):
                                final[k, j, :n].copy_(v, non_blocking=True)
                per_step.sync()

            variants = {"record": rec, "explore 0": rec0, "transitions": trans, "loop": loop}
            calls, times = {}, {name: [] for name in variants}
            for name, run in variants.items():  # warm-up, and how many calls make 100 ms
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
            trans(1)
            ended = float(((done[:, :n] | trunc[:, :n]) != 0).float().mean())
            for e in engines:
                e.close()
            out = {"ended_share": ended}
            for name, ts in times.items():
                med = float(np.median(ts))
                out[name] = {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name],
                             "lane_steps_per_s": n * K / med}
            m = lambda name: out[name]["seconds_median"]  # noqa: E731
            out["transitions_over_record"] = m("transitions") / m("record")
            out["transitions_over_loop"] = m("transitions") / m("loop")
            out["explore0_over_record"] = m("explore 0") / m("record")
            result["envs"][env]["table" if table else "uniform"] = out
            for name in variants:
                v = out[name]
                print(f"{env} | {'table' if table else 'uniform'} | {name}: {K} steps {v['seconds_median'] * 1e3:.3f} ms (min "
                      f"{v['seconds_min'] * 1e3:.3f}, max {v['seconds_max'] * 1e3:.3f}), {v['lane_steps_per_s']:.4g} lane-steps/s", flush=True)
            print(f"{env} | {'table' if table else 'uniform'} | ended share {ended:.4f}; (b)/(a) {out['transitions_over_record']:.3f}, (b)/(c) "
                  f"{out['transitions_over_loop']:.3f}, (b0)/(a) {out['explore0_over_record']:.3f}", flush=True)
    for name in sorted(resources):
        print(name, resources[name])
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
