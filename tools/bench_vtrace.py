#!/usr/bin/env python
"""gymrs_vtrace against gymrs_advantages with GYMRS_ADVANTAGES_CRITIC on the same record in the same process (profiles/vtrace.md):

    python tools/bench_vtrace.py [--shapes 1048576x16,4096x256] [--hidden 0,64] [--reps 9] [--json FILE]

CartPole; one uniform policy set and one uniform critic set of the same hidden width; a synthetic record (normal observations, 4 % of the
lane-steps done, 4 % truncated, final observations given).  The yardstick is the nearest existing launch: it does the critic's half of
the forward work (one forward pass per lane-step where V-trace does two), so the figure to compare is the time per forward pass.  Each
time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max, the two
calls taking turns.  Every measurement runs under its own time limit.  GYMRS_AMD_LIB selects another build of the library."""
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1048576x16,4096x256")
    ap.add_argument("--hidden", default="0,64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_vtrace: no GPU visible (there is no CPU fallback)")
    dev, kind, d = "cuda:0", gymrs.CARTPOLE, 4
    result = {"gpu": torch.cuda.get_device_name(0), "reps": args.reps, "cases": []}
    for shape in args.shapes.split(","):
        n, K = (int(v) for v in shape.split("x"))
        stride = (n + 15) // 16 * 16
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
        flag = lambda: (torch.rand((K, stride), device=dev, generator=g) < 0.04).to(torch.uint8)  # noqa: E731
        obs, final, start, rew = rnd(K, d, stride), rnd(K, d, stride), rnd(d, stride), rnd(K, stride)
        act = torch.randint(0, 2, (K, stride), device=dev, generator=g, dtype=torch.uint8)
        done, trunc = flag(), flag()
        po = 0.25 + 0.5 * torch.rand((K, stride), device=dev, generator=g)
        vs, pg, val, adv, ret = (torch.zeros((K, stride), device=dev) for _ in range(5))
        torch.cuda.synchronize()
        record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(), lane_stride=stride)
        eng = gymrs.BatchedEngine(kind, n, flags=gymrs.AUTO_RESET)
        eng.reset(seed=0)
        for hidden in (int(h) for h in args.hidden.split(",")):
            rng = np.random.default_rng(hidden)
            eng.set_policy((rng.standard_normal((1, gymrs.policy_size(kind, hidden))) / 2).astype(np.float32), hidden=hidden, lanes_per_policy=n)
            eng.set_critic((rng.standard_normal((1, gymrs.critic_size(kind, hidden))) / 2).astype(np.float32), hidden=hidden, lanes_per_critic=n)

            def vtrace(calls):
                for _ in range(calls):
                    eng.vtrace(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), old_prob=po.data_ptr(), vs=vs.data_ptr(),
                               pg_advantages=pg.data_ptr(), values=val.data_ptr(), gamma=0.97, lam=0.9, temperature=1.0)
                eng.sync()

            def advantages(calls):
                for _ in range(calls):
                    eng.advantages(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), advantages=adv.data_ptr(), returns=ret.data_ptr(),
                                   values=val.data_ptr(), gamma=0.97, lam=0.9, critic=True)
                eng.sync()

            variants = {"vtrace": vtrace, "advantages": advantages}
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
            out = {"n_envs": n, "steps": K, "hidden": hidden}
            for name, ts in times.items():
                out[name] = {"seconds_median": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name]}
            # two forward passes per lane-step against one
            out["vtrace_per_forward_over_advantages"] = out["vtrace"]["seconds_median"] / 2 / out["advantages"]["seconds_median"]
            result["cases"].append(out)
            print(f"{n} x {K} | H = {hidden} | " + " | ".join(f"{name} {v['seconds_median'] * 1e3:.3f} ms (min {v['seconds_min'] * 1e3:.3f}, max "
                  f"{v['seconds_max'] * 1e3:.3f})" for name, v in out.items() if isinstance(v, dict)) +
                  f" | per forward pass, vtrace / advantages = {out['vtrace_per_forward_over_advantages']:.3f}", flush=True)
        eng.close()
    if args.json:
        Path(args.json).write_text(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
