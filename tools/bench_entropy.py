#!/usr/bin/env python
"""The entropy bonus and the KL estimate over a record: gymrs_entropy_gradient against the same quantity through torch autograd
(profiles/entropy.md).  One process, taking turns, both on ONE stream (the engine rides torch's):

    python tools/bench_entropy.py [--n-envs 1048576] [--steps 64] [--reps 5] [--json FILE]

CartPole with H = 0 and H = 64 (one policy for all lanes), temperature 1, a record written by rollout_transitions(sample=True) on an
engine with A | S | T, old_prob = the prob row of weights a small step away from the ones the launch runs under.
  (a) entropy     entropy_gradient(K, record, start_obs -> grad, excluded, sums, counts): ONE launch, no action row
  (b) entropy+kl  the same with old_prob (and the action row): the KL estimate in the same launch
  (c) ppo         ppo_gradient over the same record, for scale: the launch (a) and (b) run behind
  (d) autograd    the same quantity in torch: the forward pass over the [K * n, D] observations, log_softmax, coef * sum of the entropy,
                  backward to the weights, and the k3 estimate from gather / exp / log without a gradient
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max.
Also reports (a)'s mean entropy and (b)'s KL estimate beside torch's (f32 torch against the fixed-point sums: a plausibility check,
not a test), the bytes (a) and (b) move by construction per lane-step, and the registers and scratch of every entropy kernel from the
library's code-object metadata.  Every measurement runs under its own time limit."""
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

from bench_policy_gradient import kernel_resources  # noqa: E402
from bench_policy_rollout import kernel_source_sha16  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, K = args.n_envs, args.steps
    lib_path = importlib.import_module("gym-rs_amd._lib").library_path()
    resources = {k: v for k, v in kernel_resources(lib_path, pattern=r"entropy_kernel").items()}  # before the GPU is touched

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_entropy: no GPU visible (there is no CPU fallback)")
    dev, kind, d, a, coef = "cuda:0", gymrs.CARTPOLE, 4, 2, 0.01

    def timed(run):
        """(median, min, max) seconds per call over reps repetitions of >= 100 ms"""
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
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                run(c)
                times.append((time.perf_counter() - t0) / c)
        finally:
            faulthandler.cancel_dump_traceback_later()
        return float(np.median(times)), min(times), max(times)

    result = {"gpu": torch.cuda.get_device_name(0), "kernel_source_sha16": kernel_source_sha16(), "n_envs": n, "steps": K, "reps": args.reps,
              "cases": {}, "kernels": resources}
    stride = (n + 15) // 16 * 16
    stream = torch.cuda.Stream()
    eng = gymrs.BatchedEngine(kind, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT)
    eng.set_stream(stream.cuda_stream)
    eng.reset(seed=0)
    with torch.cuda.stream(stream):
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        obs, final, start, rew = f32(K, d, stride), f32(K, d, stride), f32(d, stride), f32(K, stride)
        act, done, trunc = u8(K, stride), u8(K, stride), u8(K, stride)
        adv = torch.randn((K, stride), dtype=torch.float32, device=dev)
        old_prob = f32(K, stride)
        record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(), lane_stride=stride)
        rng = np.random.default_rng(1)
        for hidden in (0, 64):
            size = gymrs.policy_size(kind, hidden)
            w_old = (rng.standard_normal(size) / np.sqrt(max(hidden, d))).astype(np.float32)
            w_new = (w_old + 0.3 * rng.standard_normal(size) / np.sqrt(max(hidden, d))).astype(np.float32)
            grad, excl = torch.zeros((1, size), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
            sums, counts = (torch.zeros((1, 2), dtype=torch.int64, device=dev) for _ in range(2))
            eng.set_policy(w_old, hidden=hidden, lanes_per_policy=n)
            eng.set_sampling(7, temperature=1.0)
            eng.rollout_transitions(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), sample=True)
            common = dict(record=record, start_obs=start.data_ptr(), grad=grad.data_ptr(), excluded=excl.data_ptr(), temperature=1.0)
            eng.policy_gradient(K, coef=adv.data_ptr(), prob=old_prob.data_ptr(), **common)
            eng.set_policy(w_new, hidden=hidden, lanes_per_policy=n)
            eng.sync()

            def entropy(calls, kl=False):
                for _ in range(calls):
                    eng.entropy_gradient(K, sums=sums.data_ptr(), counts=counts.data_ptr(), coef=coef, old_prob=old_prob.data_ptr() if kl else None, **common)
                eng.sync()

            def ppo(calls):
                for _ in range(calls):
                    eng.ppo_gradient(K, advantages=adv.data_ptr(), old_prob=old_prob.data_ptr(), clip=0.2, **common)
                eng.sync()

            # torch's view of the record: x [K * n, D] (start_obs, then obs[0 .. K-2]), the actions and old_prob as [K * n]
            x = torch.cat([start[None, :, :n], obs[:K - 1, :, :n]]).permute(0, 2, 1).reshape(K * n, d).contiguous()
            a_t, po_t = act[:, :n].reshape(-1).long(), old_prob[:, :n].reshape(-1)
            wt = torch.from_numpy(w_new).to(dev)
            if hidden == 0:
                params = [wt[:a * d].reshape(a, d).clone().requires_grad_(), wt[a * d:].clone().requires_grad_()]
            else:
                o1, o2 = hidden * d, hidden * d + hidden
                params = [p.clone().requires_grad_() for p in (wt[:o1].reshape(hidden, d), wt[o1:o2], wt[o2:o2 + a * hidden].reshape(a, hidden),
                                                               wt[o2 + a * hidden:])]
            seen = {}

            def autograd(calls):
                for _ in range(calls):
                    for p in params:
                        p.grad = None
                    y = x @ params[0].T + params[1] if hidden == 0 else torch.relu(x @ params[0].T + params[1]) @ params[2].T + params[3]
                    logp = torch.log_softmax(y, dim=1)
                    ent = -(logp.exp() * logp).sum()
                    (coef * ent).backward()
                    with torch.no_grad():
                        ratio = logp.gather(1, a_t[:, None])[:, 0].exp() / po_t
                        seen["kl"] = ((ratio - 1) - ratio.log()).mean()
                    seen["entropy"] = ent.detach() / (K * n)
                torch.cuda.synchronize()

            case = {"hidden": hidden}
            for name, run in (("entropy", entropy), ("entropy_kl", lambda c: entropy(c, True)), ("ppo", ppo), ("autograd", autograd)):
                med, lo, hi = timed(run)
                case[name] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3}
            for t in (grad, excl, sums, counts):
                t.zero_()
            entropy(1, True)
            s, c = sums.cpu().numpy()[0], counts.cpu().numpy()[0]
            case["mean_entropy"] = {"library": float(s[0] * 2.0**-24 / c[0]), "torch": float(seen["entropy"])}
            case["kl_estimate"] = {"library": float(s[1] * 2.0**-24 / c[1]), "torch": float(seen["kl"])}
            case["excluded"] = int(excl[0])
            case["bytes_per_lane_step"] = {"entropy": 4 * d, "entropy_kl": 4 * d + 1 + 4}
            case["GB_per_s_entropy"] = 4 * d * K * n * (1 if hidden == 0 else (hidden + 3) // 4) / (case["entropy"]["ms"] * 1e-3) / 1e9
            result["cases"][f"cartpole_h{hidden}"] = case
            print(json.dumps(case))
    eng.close()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"kernels": resources}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
