#!/usr/bin/env python
"""gymrs_policy_gradient against torch autograd over the same record (profiles/policy_gradient.md).  One process, taking turns:

    python tools/bench_policy_gradient.py [--n-envs 1048576] [--steps 64] [--reps 9] [--json FILE] [--resources-only]

CartPole with H = 0, 16 and 64 and MountainCar with H = 0 (one policy and one critic for all lanes), temperature 1, a record written by
rollout_transitions(sample=True) on an engine with A | S | T, coefficients drawn once (standard normal).
  (a) fused   policy_gradient(K, record, start_obs, coef -> grad, excluded): ONE launch per head
  (b) torch   the update of examples/actor_critic_collection.py on the same tensors: einsum, log_softmax, gather, backward for the
              policy; einsum, relu, einsum, backward for the critic; the loss is sum(coef * log pi) resp. sum(coef * V), so both
              compute the same gradient.
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max.
Also reports the bytes moved by construction per lane-step for the affine networks and the share of this box's copy rate (a 1 GiB
device copy timed in the same process) they make, the largest difference of each gradient to f64 autograd (2^16 lanes at a time) beside the largest entry,
and the registers and scratch of every gradient kernel from the library's code-object metadata (`--resources-only`: nothing else,
no GPU).  Every measurement runs under its own time limit."""
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
LIMIT_S = 180  # per measurement

from bench_policy_rollout import kernel_source_sha16  # noqa: E402


def kernel_resources(lib: Path) -> dict:
    """VGPR / AGPR / SGPR / scratch / spill counts of gradient_kernel<..>, from the code-object metadata (no GPU needed).  Called
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
            for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                name = re.search(r"\.name:\s+(\S*gradient_(?:ppo_)?kernel\S*)", block)  # gymrs_policy_gradient's and gymrs_ppo_gradient's
                if not name:
                    continue
                field = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))  # noqa: E731
                nice = subprocess.run(["c++filt", name.group(1)], capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout.strip() or name.group(1)
                nice = re.sub(r"\(.*$", "", nice).replace("void gymrs::", "").replace("gymrs::", "")
                out[nice] = {"vgpr": field("vgpr_count"), "agpr": int(re.match(r"\s*(\d+)", block).group(1)), "sgpr": field("sgpr_count"),
                             "scratch_bytes": field("private_segment_fixed_size"), "vgpr_spill": field("vgpr_spill_count"), "sgpr_spill": field("sgpr_spill_count")}
    return out


def bytes_per_lane_step(d: int, critic: bool) -> int:
    """by construction, affine networks: one read of the observation, the coefficient and (policy head) the action; S sums out"""
    return 4 * d + 4 + (0 if critic else 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
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
        raise SystemExit("bench_policy_gradient: no GPU visible (there is no CPU fallback)")
    dev = "cuda:0"
    A_S_T = gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT

    def timed(run, reps):
        """(per-call times of `reps` repetitions of >= 100 ms, calls per repetition)"""
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

    # the yardstick: a 1 GiB device copy (reads and writes 1 GiB each)
    src, dst = torch.empty(1 << 28, dtype=torch.float32, device=dev), torch.empty(1 << 28, dtype=torch.float32, device=dev)

    def copy(calls):
        for _ in range(calls):
            dst.copy_(src)
        torch.cuda.synchronize()

    c = timed(copy, 1)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        copy(c)
        ts.append((time.perf_counter() - t0) / c)
    copy_rate = 2 * (1 << 30) / float(np.median(ts))
    del src, dst
    torch.cuda.empty_cache()
    print(f"copy yardstick: {copy_rate / 1e12:.3f} TB/s (1 GiB device copy, read + write)", flush=True)

    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "library": str(lib_path.name), "n_envs": n, "steps": K,
              "reps": args.reps, "copy_bytes_per_s": copy_rate, "cases": {}, "kernels": resources}
    stride = (n + 15) // 16 * 16
    scale = 1.4426950408889634
    for env, kind, hiddens in (("cartpole", gymrs.CARTPOLE, (0, 16, 64)), ("mountain_car", gymrs.MOUNTAIN_CAR, (0,))):
        d, a_n = (4, 2) if kind == gymrs.CARTPOLE else (2, 3)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        obs, final, start, rew = f32(K, d, stride), f32(K, d, stride), f32(d, stride), f32(K, stride)
        act, done, trunc = u8(K, stride), u8(K, stride), u8(K, stride)
        coef = torch.randn((K, stride), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                      lane_stride=stride)
        rng = np.random.default_rng(1)
        eng = gymrs.BatchedEngine(kind, n, flags=A_S_T)
        eng.reset(seed=0)
        for hidden in hiddens:
            wp = (rng.standard_normal(gymrs.policy_size(kind, hidden)) / np.sqrt(max(hidden, d))).astype(np.float32)
            wc = (rng.standard_normal(gymrs.critic_size(kind, hidden)) / np.sqrt(max(hidden, d))).astype(np.float32)
            eng.set_policy(wp, hidden=hidden, lanes_per_policy=n)
            eng.set_critic(wc, hidden=hidden, lanes_per_critic=n)
            eng.set_sampling(7, temperature=1.0)
            eng.rollout_transitions(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), sample=True)
            eng.sync()
            for critic in (False, True):
                w = wc if critic else wp
                outs = 1 if critic else a_n
                grad = torch.zeros((1, w.size), dtype=torch.int64, device=dev)
                excl = torch.zeros(1, dtype=torch.int64, device=dev)
                wt = torch.from_numpy(w).to(dev)
                torch.cuda.synchronize()

                def fused(calls):
                    for _ in range(calls):
                        eng.policy_gradient(K, record=record, start_obs=start.data_ptr(), coef=coef.data_ptr(), grad=grad.data_ptr(), excluded=excl.data_ptr(),
                                            critic=critic, scale=None if critic else scale)
                    eng.sync()

                last = {}

                def torch_gradient(dtype, lo, hi):
                    theta = wt.detach().to(dtype).clone().requires_grad_(True)
                    s = torch.cat([start[None, :, lo:hi], obs[:-1, :, lo:hi]]).to(dtype)
                    if hidden == 0:
                        y = torch.einsum("aj,kjn->kan", theta[:outs * d].reshape(outs, d), s) + theta[outs * d:][None, :, None]
                    else:
                        h = hidden
                        w1, b1 = theta[:h * d].reshape(h, d), theta[h * d:h * d + h]
                        w2, b2 = theta[h * d + h:h * d + h + outs * h].reshape(outs, h), theta[h * d + h + outs * h:]
                        y = torch.einsum("ah,khn->kan", w2, torch.relu(torch.einsum("hj,kjn->khn", w1, s) + b1[None, :, None])) + b2[None, :, None]
                    out = y[:, 0] if critic else torch.log_softmax(y, dim=1).gather(1, act[:, lo:hi].long()[:, None, :]).squeeze(1)
                    (out * coef[:, lo:hi].to(dtype)).sum().backward()
                    return theta.grad

                def autograd(calls):
                    for _ in range(calls):
                        last["grad"] = torch_gradient(torch.float32, 0, n)
                    torch.cuda.synchronize()

                def gradient64():  # the yardstick of the comparison: f64 autograd, 2^16 lanes at a time
                    total = torch.zeros(w.size, dtype=torch.float64, device=dev)
                    for lo in range(0, n, 1 << 16):
                        total += torch_gradient(torch.float64, lo, min(n, lo + (1 << 16)))
                    return total

                variants = {"fused": fused, "torch": autograd}
                label = f"{env} H={hidden} {'critic' if critic else 'policy'}"
                calls, times = {}, {name: [] for name in variants}
                try:
                    for name, run in variants.items():
                        calls[name] = timed(run, args.reps)
                except torch.cuda.OutOfMemoryError as err:  # the [K, H, n] intermediates of autograd
                    print(f"{label}: torch ran out of memory: {str(err)[:120]}", flush=True)
                    variants.pop("torch")
                    torch.cuda.empty_cache()
                for _ in range(args.reps):  # taking turns
                    for name, run in variants.items():
                        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
                        try:
                            t0 = time.perf_counter()
                            run(calls[name])
                            times[name].append((time.perf_counter() - t0) / calls[name])
                        finally:
                            faulthandler.cancel_dump_traceback_later()
                grad.zero_()
                excl.zero_()
                torch.cuda.synchronize()
                fused(1)
                mine = grad[0].double() * 2.0**-24
                out = {"excluded": int(excl[0])}
                exact = gradient64()
                out["largest_entry"] = float(exact.abs().max())
                out["fused_vs_f64"] = float((mine - exact).abs().max())
                if "grad" in last:
                    out["torch_vs_f64"] = float((last["grad"].double() - exact).abs().max())
                for name in variants:
                    ts = times[name]
                    med = float(np.median(ts))
                    out[name] = {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name]}
                    print(f"{label} | {name}: {med * 1e3:.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f})", flush=True)
                if hidden == 0:
                    b = bytes_per_lane_step(d, critic)
                    rate = b * n * K / out["fused"]["seconds_median"]
                    out["bytes_per_lane_step"], out["fused_bytes_per_s"], out["share_of_copy_rate"] = b, rate, rate / copy_rate
                    print(f"{label} | {b} B per lane-step by construction: {rate / 1e12:.3f} TB/s, {rate / copy_rate:.3f} of the copy rate", flush=True)
                if "torch" in variants:
                    out["fused_over_torch"] = out["fused"]["seconds_median"] / out["torch"]["seconds_median"]
                    print(f"{label} | fused / torch {out['fused_over_torch']:.4f}", flush=True)
                print(f"{label} | largest difference to f64 autograd: fused {out['fused_vs_f64']:.3g}, torch f32 {out.get('torch_vs_f64', float('nan')):.3g}, of largest "
                      f"entry {out['largest_entry']:.3g}; excluded {out['excluded']}", flush=True)
                result["cases"][label] = out
                last.clear()
                torch.cuda.empty_cache()
        eng.close()
        del obs, final, start, rew, act, done, trunc, coef
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
