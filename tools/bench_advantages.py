#!/usr/bin/env python
"""gymrs_advantages against the backward loop users write today (profiles/advantages.md).  One process, the two taking turns:

    python tools/bench_advantages.py [--n-envs 1048576] [--steps 64] [--reps 9] [--json FILE]

CartPole and MountainCar; the critic off, affine, H = 16 and H = 64 (one critic for all lanes); gamma 0.97, lambda 0.9; a record
written by rollout_transitions(sample=True) on an engine with A | S | T and its default episode limits.
  (a) fused   advantages(K, record, final_obs, start_obs -> advantages, returns, values): ONE launch
  (b) torch   the loop of examples/policy_gradient_collection.py extended to GAE with a batched torch critic on the same tensors:
              V over all K + 1 observation rows and over final_obs in a few large torch calls, then
              `for k in range(K - 1, -1, -1)` with the three-way case split written as torch.where.  This is what users write
              today, so it is the baseline.
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max.
Also reports the bytes moved by construction per lane-step, the HBM rate that makes at the fused median, and the registers and
scratch of every advantages kernel from the library's code-object metadata.  Every measurement runs under its own time limit.
GYMRS_AMD_LIB selects another build of the library."""
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
    """VGPR / SGPR / scratch / spill counts of advantages_kernel<..>, from the code-object metadata (no GPU needed).  Called before
    the HIP runtime is up: it starts child processes."""
    llvm = next((d for d in (Path("/opt/rocm/llvm/bin"), Path(shutil.which("llvm-readelf") or "/nonexistent").parent) if (d / "llvm-readelf").exists()), None)
    if llvm is None:
        return {"error": "llvm-readelf not found"}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, Path(tmp) / "lib.so")
        subprocess.run([str(llvm / "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True, stdin=subprocess.DEVNULL)
        for co in sorted(Path(tmp).glob("lib.so.*amdgcn*")):
            notes = subprocess.run([str(llvm / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout
            pat = (r"\.name:\s+(\S*advantages_kernel\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+)"
                   r".*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)")
            for m in re.finditer(pat, notes, re.S):
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout.strip() or m.group(1)
                name = re.sub(r"\(.*$", "", name).replace("void gymrs::", "").replace("gymrs::", "")
                out[name] = {"vgpr": int(m.group(5)), "sgpr": int(m.group(3)), "scratch_bytes": int(m.group(2)),
                             "vgpr_spill": int(m.group(6)), "sgpr_spill": int(m.group(4))}
    return out


def bytes_per_lane_step(d: int, critic: bool) -> dict:
    """by construction: one read of the record, one write of the three outputs; without a critic no observation is read"""
    return {"read": (4 * d if critic else 0) + 4 + 1 + 1, "written": 12}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, K = args.n_envs, args.steps
    gamma, lam = 0.97, 0.9
    lib_path = importlib.import_module("gym-rs_amd._lib").library_path()
    resources = kernel_resources(lib_path)  # before the GPU is touched

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_advantages: no GPU visible (there is no CPU fallback)")
    dev = "cuda:0"
    A_S_T = gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT
    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "library": str(lib_path.name), "n_envs": n, "steps": K,
              "gamma": gamma, "lambda": lam, "reps": args.reps, "envs": {}, "kernels": resources}
    stride = (n + 15) // 16 * 16
    for env, kind in (("cartpole", gymrs.CARTPOLE), ("mountain_car", gymrs.MOUNTAIN_CAR)):
        d = 4 if kind == gymrs.CARTPOLE else 2
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        obs, final, start, rew = f32(K, d, stride), f32(K, d, stride), f32(d, stride), f32(K, stride)
        act, done, trunc = u8(K, stride), u8(K, stride), u8(K, stride)
        adv, ret, val = f32(K, stride), f32(K, stride), f32(K, stride)
        torch.cuda.synchronize()
        record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                      lane_stride=stride)
        rng = np.random.default_rng(1)
        eng = gymrs.BatchedEngine(kind, n, flags=A_S_T)
        eng.reset(seed=0)
        eng.set_policy(rng.standard_normal((1, gymrs.policy_size(kind, 0))).astype(np.float32), hidden=0, lanes_per_policy=n)
        eng.set_sampling(7, temperature=1.0)
        eng.rollout_transitions(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), sample=True)
        eng.sync()
        ended_share = float(((done[:, :n] | trunc[:, :n]) != 0).float().mean())
        result["envs"][env] = {"ended_share": ended_share}
        for label, hidden in (("no critic", None), ("affine", 0), ("H=16", 16), ("H=64", 64)):
            critic = hidden is not None
            if critic:
                size = gymrs.critic_size(kind, hidden)
                w = (rng.standard_normal(size) / np.sqrt(max(hidden, d))).astype(np.float32)
                eng.set_critic(w, hidden=hidden, lanes_per_critic=n)
                wt = torch.from_numpy(w).to(dev)
                if hidden == 0:
                    w1, b1 = wt[:d].reshape(1, d), wt[d:]
                    w2 = b2 = None
                else:
                    w1, b1 = wt[:hidden * d].reshape(hidden, d), wt[hidden * d:hidden * d + hidden]
                    w2, b2 = wt[hidden * d + hidden:hidden * d + 2 * hidden], wt[-1]
                torch.cuda.synchronize()

            def value(x):  # x [rows][d][n] -> [rows][n]: the batched torch critic
                z = torch.einsum("hj,kjn->khn", w1, x) + b1[None, :, None]
                if w2 is None:
                    return z[:, 0]
                return torch.einsum("h,khn->kn", w2, torch.relu(z)) + b2

            def fused(calls):
                for _ in range(calls):
                    eng.advantages(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), advantages=adv.data_ptr(),
                                   returns=ret.data_ptr(), values=val.data_ptr(), gamma=gamma, lam=lam, critic=critic)
                eng.sync()

            out_a, out_r = f32(K, n), f32(K, n)

            def loop(calls):
                for _ in range(calls):
                    dn, tr = done[:, :n] != 0, trunc[:, :n] != 0
                    ended = dn | tr
                    if critic:
                        v_all = value(torch.cat([start[None, :, :n], obs[:, :, :n]]))  # V(s_0 .. s_K)
                        v_fin = value(final[:, :, :n])
                        v_cur, v_obs = v_all[:-1], v_all[1:]
                        v_next = torch.where(dn, 0.0, torch.where(ended, v_fin, v_obs))
                    else:
                        v_cur = v_next = torch.zeros((K, n), device=dev)
                    run = torch.zeros(n, device=dev)
                    for k in range(K - 1, -1, -1):
                        delta = rew[k, :n] + gamma * v_next[k] - v_cur[k]
                        run = delta + gamma * lam * torch.where(ended[k], 0.0, run)
                        out_a[k] = run
                    torch.add(out_a, v_cur, out=out_r)
                torch.cuda.synchronize()

            variants = {"fused": fused, "torch": loop}
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
            # the two agree (f32 rounding apart: the torch critic sums in another order)
            finite = torch.isfinite(out_a)
            worst = float((adv[:, :n] - out_a)[finite].abs().max())
            out = {"max_abs_difference_fused_vs_torch": worst, "bytes_per_lane_step": bytes_per_lane_step(d, critic)}
            for name, ts in times.items():
                med = float(np.median(ts))
                out[name] = {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name],
                             "lane_steps_per_s": n * K / med}
            b = out["bytes_per_lane_step"]
            out["fused_over_torch"] = out["fused"]["seconds_median"] / out["torch"]["seconds_median"]
            out["fused_bytes_per_s"] = (b["read"] + b["written"]) * n * K / out["fused"]["seconds_median"]
            result["envs"][env][label] = out
            for name in variants:
                v = out[name]
                print(f"{env} | {label} | {name}: K = {K}: {v['seconds_median'] * 1e3:.3f} ms (min {v['seconds_min'] * 1e3:.3f}, max "
                      f"{v['seconds_max'] * 1e3:.3f}), {v['lane_steps_per_s']:.4g} lane-steps/s", flush=True)
            print(f"{env} | {label} | fused / torch {out['fused_over_torch']:.4f}; {b['read']} + {b['written']} B per lane-step by construction: "
                  f"{out['fused_bytes_per_s'] / 1e12:.3f} TB/s; max |fused - torch| {worst:.3g}; ended share {ended_share:.4f}", flush=True)
        eng.close()
        del obs, final, start, rew, act, done, trunc, adv, ret, val
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
