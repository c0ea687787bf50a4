#!/usr/bin/env python
"""Truncation bootstrapping with GYMRS_FINAL_OBS, zero-copy from PyTorch.

Pendulum never terminates: every episode ends at the time limit (`truncated`), and the engine re-arms the lane inside the
same step (GYMRS_AUTO_RESET), so after the step `obs` already shows the NEW episode.  A TD / GAE target of a truncated step
must bootstrap from the observation the old episode ended in; GYMRS_FINAL_OBS keeps it in device arrays of its own:

    target = r + gamma * (1 - done) * V(where(truncated, final_obs, obs))

Every array below is the engine's own device memory wrapped as a torch tensor (CUDA array interface): no copies, one stream.
The critic is a fixed quadratic stand-in; any torch module works the same way.

    python examples/truncation_bootstrap.py [--n-envs 1048576] [--steps 600]
"""
from __future__ import annotations

import argparse
import importlib
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
gymrs = importlib.import_module("gym-rs_amd")


class DeviceColumn:
    """A device array owned by the engine, presented to torch without a copy."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def column(ptr: int, n: int, typestr: str = "<f4") -> torch.Tensor:
    return torch.as_tensor(DeviceColumn(ptr, n, typestr), device="cuda:0")


def critic(obs: torch.Tensor) -> torch.Tensor:
    """V(s) for Pendulum observations (cos, sin, theta_dot) stacked as (3, n): a stand-in for a learned value function."""
    cos, _, theta_dot = obs
    return -4.0 * (1.0 - cos) - 0.1 * theta_dot * theta_dot


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--gamma", type=float, default=0.99)
    args = ap.parse_args()
    n = args.n_envs

    stream = torch.cuda.Stream()
    env = gymrs.BatchedEngine(gymrs.PENDULUM, n, flags=gymrs.AUTO_RESET | gymrs.TIME_LIMIT | gymrs.FINAL_OBS)
    env.set_stream(stream.cuda_stream)  # the engine launches on torch's stream: no synchronisation between step and learner
    env.reset(seed=0)
    obs = [column(p, n) for p in env.obs_ptrs()]              # (cos, sin, theta_dot) after the step
    final_obs = [column(p, n) for p in env.final_obs_ptrs()]  # where each lane's last finished episode ended
    reward = column(env.reward_ptr, n)
    done = column(env.done_ptr, n, "|u1")
    truncated = column(env.truncated_ptr, n, "|u1")
    action = torch.empty(n, dtype=torch.float32, device="cuda:0")
    target = torch.empty(n, dtype=torch.float32, device="cuda:0")
    boot_gap = torch.zeros((), dtype=torch.float64, device="cuda:0")
    n_truncated = torch.zeros((), dtype=torch.int64, device="cuda:0")

    with torch.cuda.stream(stream):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            # policy: torque against the angular velocity, clipped to the action box
            torch.clamp(-2.0 * obs[2], -2.0, 2.0, out=action)
            env.step(action.data_ptr())
            trunc = truncated.bool()
            next_obs = torch.where(trunc, torch.stack(final_obs), torch.stack(obs))
            torch.add(reward, args.gamma * (1.0 - done.float()) * critic(next_obs), out=target)
            # what bootstrapping from the re-armed state instead would have changed, summed over the truncated lanes
            boot_gap += torch.where(trunc, critic(torch.stack(final_obs)) - critic(torch.stack(obs)), 0.0).abs().sum()
            n_truncated += trunc.sum()
        env.sync()
        dt = time.perf_counter() - t0
    k = int(n_truncated)
    print(f"{n} envs x {args.steps} steps in {dt * 1e3:.1f} ms (targets included); truncated lane-steps {k}")
    if k:
        print(f"mean |V(final_obs) - V(obs)| over truncated lane-steps: {float(boot_gap) / k:.3f}"
              " (the error a target makes that bootstraps from the re-armed state)")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
