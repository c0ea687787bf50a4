#!/usr/bin/env python
"""Actor-critic on CartPole with several optimiser steps per record, the targets corrected by V-trace before each of them.

One `rollout_transitions` record, then E epochs of `vtrace` -> `value_gradient` / `policy_gradient` -> `apply_gradient` (both heads).
After the first update the record is off-policy: every epoch's `vtrace` reads the record's ORIGINAL prob row as `old_prob` and the
engine's current weights, so the targets follow the policy as it moves.  The engine rides torch's stream and nothing inside the epoch
loop waits for the device; the clip counters of every epoch go to a row of their own and are read once per round.

    python examples/vtrace_actor_critic.py [--lanes 4096] [--steps 64] [--rounds 8] [--epochs 4] [--limit 100] [--hidden 16]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64, help="K: steps per launch")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=4, help="E: optimiser steps on one record")
    ap.add_argument("--limit", type=int, default=100, help="max_episode_steps")
    ap.add_argument("--hidden", type=int, default=16, help="H of both networks (0: affine)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    n, steps, H, E, dev = args.lanes, args.steps, args.hidden, args.epochs, "cuda:0"
    gamma, lam, lr_pi, lr_v = 0.97, 1.0, 0.02, 0.01
    rng = np.random.default_rng(args.seed)
    policy = (0.1 * rng.standard_normal(gymrs.policy_size(gymrs.CARTPOLE, H))).astype(np.float32)
    critic = (0.1 * rng.standard_normal(gymrs.critic_size(gymrs.CARTPOLE, H))).astype(np.float32)

    params = gymrs.engine.default_params(gymrs.CARTPOLE)
    params.max_episode_steps = args.limit
    stream = torch.cuda.Stream()
    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT, params=params)
    env.set_stream(stream.cuda_stream)  # the engine launches on torch's stream
    env.reset(seed=args.seed)
    env.set_policy(policy, hidden=H, lanes_per_policy=n)
    env.set_critic(critic, hidden=H, lanes_per_critic=n)
    env.set_sampling(4321, temperature=1.0)

    stride = (n + 15) // 16 * 16
    grad_scale = 2.0**-24 / (steps * n)  # the tables hold sums over K * n lane-steps in units of 2^-24
    with torch.cuda.stream(stream):
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        obs, final, start, rew = f32(steps, 4, stride), f32(steps, 4, stride), f32(4, stride), f32(steps, stride)
        act, done, trunc = u8(steps, stride), u8(steps, stride), u8(steps, stride)
        vs, pg, old_prob, ones = f32(steps, stride), f32(steps, stride), f32(steps, stride), f32(steps, stride) + 1.0
        g_pi, g_v = (torch.zeros((1, t.size), dtype=torch.int64, device=dev) for t in (policy, critic))
        x_pi, x_v, skipped = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(3))
        counts = torch.zeros((E, 1, 3), dtype=torch.int64, device=dev)  # a row per epoch: lane-steps seen, rho clipped, c clipped
        record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                      lane_stride=stride)
        rows = dict(record=record, start_obs=start.data_ptr())
        targets = dict(final_obs=final.data_ptr(), vs=vs.data_ptr(), pg_advantages=pg.data_ptr(), gamma=gamma, lam=lam, temperature=1.0, **rows)

        for r in range(args.rounds):
            env.rollout_transitions(steps, final_obs=final.data_ptr(), sample=True, **rows)
            # the record's own prob row: p[a] under the weights it was drawn from (old_prob = 1 here; vs and pg are overwritten below)
            env.vtrace(steps, old_prob=ones.data_ptr(), prob=old_prob.data_ptr(), **targets)
            counts.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for e in range(E):  # nothing in here waits for the device
                env.vtrace(steps, old_prob=old_prob.data_ptr(), counts=counts[e].data_ptr(), rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, **targets)
                env.value_gradient(steps, returns=vs.data_ptr(), grad=g_v.data_ptr(), excluded=x_v.data_ptr(), **rows)
                env.policy_gradient(steps, coef=pg.data_ptr(), grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(), temperature=1.0, **rows)
                env.apply_gradient(grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(), skipped=skipped.data_ptr(), adam=True, lr=lr_pi, grad_scale=grad_scale,
                                   ascend=True, zero_grad=True)
                env.apply_gradient(grad=g_v.data_ptr(), excluded=x_v.data_ptr(), skipped=skipped.data_ptr(), critic=True, adam=True, lr=lr_v,
                                   grad_scale=grad_scale, max_norm=10.0, zero_grad=True)
            torch.cuda.synchronize()
            epoch_ms = (time.perf_counter() - t0) * 1e3 / max(1, E)

            clipped = [int(c[0, 1]) / max(1, int(c[0, 0])) for c in counts.cpu()]
            env.rollout_closed_loop(steps, fitness=True)  # greedy validation with the new weights
            reward_sum, episodes, _, _ = env.policy_fitness()[0]
            env.policy_fitness_clear()
            print(f"round {r:2d}: {steps * n} sampled transitions, share of lane-steps with ratio > rho_bar per epoch "
                  f"{' '.join(f'{f:.3f}' for f in clipped)}, {int(skipped[0])} updates skipped so far, {epoch_ms:.3f} ms per epoch; greedy validation: "
                  f"{int(reward_sum) / max(1, int(episodes) + n):.1f} steps per episode")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
