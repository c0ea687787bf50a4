#!/usr/bin/env python
"""gymrs_replay_sample and gymrs_replay_push beside the same work written with torch on the same device (profiles/replay.md).

    python tools/bench_replay.py [--capacity 4194304] [--samples 65536] [--steps 16] [--reps 5] [--json FILE]

CartPole.  A full store of `capacity` entries with random priorities in [1, 2^24]; one draw of `samples` entries with its gather;
one push of `steps` x `samples` lanes (an engine of n_envs = samples, a record written by rollout_transitions).
  draw / push          the library's calls (three launches / one launch)
  torch draw           cumsum (int64), the strata and their points in int64, searchsorted, 2 D + 4 index gathers
  torch push           the flattening with where() and one index_copy_ per row
Each time is the median of `reps` repetitions of >= 100 ms (host clock around calls that end in a synchronise), with min and max,
taking turns.  Every measurement runs under its own time limit."""
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
TILE = 4096


def draw_bytes(capacity: int, samples: int, d: int) -> dict:
    """by construction: the priorities are read twice (tile sums, then the prefix), the tile sums and bases once each way, and a sample
    reads its 2 D + 3 values and its priority and writes them with its index"""
    tiles = (capacity + TILE - 1) // TILE
    per_sample = (2 * d + 1) * 4 + 2 + 4
    return {"priorities": 2 * 4 * capacity, "scratch": 4 * 8 * tiles, "gather_read": per_sample * samples, "gather_write": (per_sample + 4) * samples}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--samples", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    cap, B, K = args.capacity, args.samples, args.steps

    import numpy as np
    import torch

    gymrs = importlib.import_module("gym-rs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay: no GPU visible (there is no CPU fallback)")
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
    stride = (B + 15) // 16 * 16
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    st = dict(s=torch.randn((d, cap), device=dev), s_next=torch.randn((d, cap), device=dev), action=u8(cap), reward=torch.randn(cap, device=dev), done=u8(cap),
              priority=torch.randint(1, (1 << 24) + 1, (cap,), dtype=torch.int32, device=dev))
    store = gymrs.Replay(*(st[k].data_ptr() for k in ("s", "s_next", "action", "reward", "done", "priority")), cap)
    store.count = cap
    obs, final, start, rew = f32(K, d, stride), f32(K, d, stride), f32(d, stride), f32(K, stride)
    act, done, trunc = u8(K, stride), u8(K, stride), u8(K, stride)
    b_obs, b_start, b_rew, b_act, b_done = f32(d, stride), f32(d, stride), f32(stride), u8(stride), u8(stride)
    idx, prio = torch.zeros(stride, dtype=torch.int32, device=dev), torch.zeros(stride, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(), lane_stride=stride)
    batch = dict(obs=b_obs.data_ptr(), actions=b_act.data_ptr(), reward=b_rew.data_ptr(), done=b_done.data_ptr(), lane_stride=stride)
    eng = gymrs.BatchedEngine(kind, B, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT)
    eng.reset(seed=0)
    eng.set_policy(np.zeros(gymrs.policy_size(kind, 0), np.float32), lanes_per_policy=B)
    eng.set_exploration(7, epsilon=1.0)
    eng.rollout_transitions(K, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), explore=True)
    eng.sync()

    def draw(calls):
        for c in range(calls):
            eng.replay_sample(store, B, seed=1, draw=c, batch=batch, start_obs=b_start.data_ptr(), idx=idx.data_ptr(), prio=prio.data_ptr(), total=total.data_ptr())
        eng.sync()

    def push(calls):
        for _ in range(calls):
            eng.replay_push(store, K, record=record, start_obs=start.data_ptr(), final_obs=final.data_ptr(), head=store.head)
        eng.sync()

    j = torch.arange(B, dtype=torch.int64, device=dev)

    def torch_draw(calls):
        for _ in range(calls):
            prefix = torch.cumsum(st["priority"], 0, dtype=torch.int64)
            T = prefix[-1]
            q, rem = T // B, T % B
            r = torch.randint(0, 1 << 32, (B,), dtype=torch.int64, device=dev)
            u = torch.minimum(j * q + torch.minimum(j, rem) + ((r * (q + (j < rem))) >> 32), T - 1)  # (r * w < 2^63 at these sizes)
            e = torch.searchsorted(prefix, u, right=True)
            out = [st["s"][:, e], st["s_next"][:, e], st["action"][e], st["reward"][e], st["done"][e], st["priority"][e]]
        torch.cuda.synchronize()
        return out

    def torch_push(calls):
        for _ in range(calls):
            at = (store.head + torch.arange(K * B, dtype=torch.int64, device=dev)) % cap
            ended = ((done != 0) | (trunc != 0))[:, None, :B]
            x = torch.cat([start[None, :, :B], obs[:-1, :, :B]]).permute(1, 0, 2).reshape(d, K * B)
            xn = torch.where(ended, final[:, :, :B], obs[:, :, :B]).permute(1, 0, 2).reshape(d, K * B)
            st["s"].index_copy_(1, at, x)
            st["s_next"].index_copy_(1, at, xn)
            st["action"].index_copy_(0, at, act[:, :B].reshape(-1))
            st["reward"].index_copy_(0, at, rew[:, :B].reshape(-1))
            st["done"].index_copy_(0, at, (done[:, :B] != 0).to(torch.uint8).reshape(-1))
            st["priority"].index_fill_(0, at, 1 << 24)
        torch.cuda.synchronize()

    variants = {"torch draw": torch_draw, "draw": draw, "torch push": torch_push, "push": push}
    calls = {name: calibrate(run) for name, run in variants.items()}
    times = {name: [] for name in variants}
    for _ in range(args.reps):  # taking turns
        for name, run in variants.items():
            times[name].append(timed(run, calls[name]) / calls[name])
    result = {"gpu": torch.cuda.get_device_name(0), "capacity": cap, "samples": B, "steps": K, "reps": args.reps, "draw_bytes": draw_bytes(cap, B, d),
              "push_bytes": K * B * (16 * d + 17), "cases": {}}
    for name, ts in times.items():
        result["cases"][name] = {"seconds_median": float(np.median(ts)), "seconds_min": min(ts), "seconds_max": max(ts), "calls_per_rep": calls[name]}
        print(f"{name}: {np.median(ts) * 1e6:.1f} us (min {min(ts) * 1e6:.1f}, max {max(ts) * 1e6:.1f})", flush=True)
    eng.close()
    print(json.dumps(result))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
