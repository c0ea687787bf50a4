#!/usr/bin/env python
"""Domain randomisation with a parameter table: every CartPole lane gets its own physics, and a finished lane draws a new row.

In gym-rs a Vec<CartPoleEnv> can give each env its own pub fields (`envs[i].length = l`).  Here one engine holds K rows of
CartPoleParams (gymrs_set_param_table) and a uint16 row index per lane in device memory; lane i steps with row index[i].  After
every step the indices of the lanes that just finished are redrawn by torch on the engine's stream, through zero-copy views of
the engine's `done` and index arrays: the next episode of such a lane runs with new physics, and nothing leaves the device.

    python examples/domain_randomization.py [--n-envs 1048576] [--rows 16] [--steps 500]
"""
from __future__ import annotations

import argparse
import importlib
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
gymrs = importlib.import_module("gym-rs_amd")


class DeviceColumn:
    """A device array owned by the engine, presented to torch without a copy."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def column(ptr: int, n: int, typestr: str) -> torch.Tensor:
    return torch.as_tensor(DeviceColumn(ptr, n, typestr), device="cuda:0")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--steps", type=int, default=500)
    args = ap.parse_args()
    n, k = args.n_envs, args.rows
    if not 1 <= k <= 64:
        ap.error("--rows: 1 .. 64 (the per-row tallies below compare every lane with every row)")

    rng = np.random.default_rng(0)
    rows = []
    for _ in range(k):  # gravity, pole length and pole mass within +-50 % of the reference's defaults
        p = gymrs.engine.default_params(gymrs.CARTPOLE)
        p.gravity *= rng.uniform(0.5, 1.5)
        p.length *= rng.uniform(0.5, 1.5)
        p.masspole *= rng.uniform(0.5, 1.5)
        rows.append(p)

    stream = torch.cuda.Stream()
    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET)
    env.set_stream(stream.cuda_stream)  # the engine launches on torch's stream: no synchronisation between step and redraw
    env.set_param_table(rows)
    index = column(env.param_index_ptr(), n, "<i2")  # (int16 view of the uint16 index: rows < 32768)
    done = column(env.done_ptr, n, "|u1")
    actions = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    row_ids = torch.arange(k, dtype=torch.int16, device="cuda:0").unsqueeze(1)
    lengths = torch.zeros(k, dtype=torch.int64, device="cuda:0")   # sum of finished episode lengths per row
    episodes = torch.zeros(k, dtype=torch.int64, device="cuda:0")  # finished episodes per row
    age = torch.zeros(n, dtype=torch.int32, device="cuda:0")       # steps in each lane's open episode

    with torch.cuda.stream(stream):
        index.copy_(torch.randint(0, k, (n,), device="cuda:0", generator=gen, dtype=torch.int16))
        env.reset(seed=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(args.steps):
            env.fill_actions(actions.data_ptr(), seed=7, t=t)
            env.step(actions.data_ptr())
            age += 1
            fin = done.bool()
            hit = (index.unsqueeze(0) == row_ids) & fin  # (k, n): the lanes of row r whose episode ended in this step
            lengths += torch.where(hit, age, 0).sum(1)
            episodes += hit.sum(1)
            age.masked_fill_(fin, 0)
            # the finished lanes' next episode gets a new row: read by the next step, in stream order
            fresh = torch.randint(0, k, (n,), device="cuda:0", generator=gen, dtype=torch.int16)
            index.copy_(torch.where(fin, fresh, index))
        env.sync()
        dt = time.perf_counter() - t0
    print(f"{n} envs x {args.steps} steps with {k} physics rows in {dt * 1e3:.1f} ms (redraws included)")
    print(" row  gravity  length  masspole  episodes  mean length")
    for r, p in enumerate(rows):
        e = int(episodes[r])
        print(f"{r:4d} {p.gravity:8.3f} {p.length:7.3f} {p.masspole:9.4f} {e:9d} {int(lengths[r]) / max(e, 1):12.2f}")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
