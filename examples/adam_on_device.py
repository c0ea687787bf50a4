#!/usr/bin/env python
"""PPO on CartPole with the weight update inside the library too: the loop of `examples/ppo_cartpole.py` with
`apply_gradient(adam=True, zero_grad=True)` in place of the torch update.

The engine rides torch's stream.  The advantages are normalised by `normalize_advantages` once per round, and an epoch is four or
five launches with no torch expression in between: `ppo_gradient`, (`entropy_gradient`,) `value_gradient` -- the critic head with
its coefficient V - R computed in the kernel from V under the current critic, so no values row has to be refreshed --, and one
`apply_gradient` per head (Adam from the fixed-point tables into the engine's own weights; the tables come back zeroed for the next
epoch).  No `torch.cuda.synchronize()` inside the epoch loop, no memset, no optimizer state outside the engine.  The counters of
every epoch go to a row of their own and are read once per round.

    python examples/adam_on_device.py [--lanes 4096] [--steps 64] [--rounds 8] [--epochs 4] [--clip 0.2] [--clip-vf X] [--limit 100] [--hidden 16]
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
    ap.add_argument("--epochs", type=int, default=4, help="E: passes over one record")
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--clip-vf", type=float, default=None, help="clip the value loss within X of the values the record was scored with (GYMRS_VALUE_CLIP)")
    ap.add_argument("--limit", type=int, default=100, help="max_episode_steps")
    ap.add_argument("--hidden", type=int, default=16, help="H of the critic (0: affine)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--entropy", type=float, default=0.0, help="c_ent: the entropy bonus coefficient (entropy_gradient into the policy's table)")
    ap.add_argument("--target-kl", type=float, default=None, help="report the k3 KL estimate of every epoch and the first epoch beyond this value")
    args = ap.parse_args()
    with_entropy = args.entropy != 0.0 or args.target_kl is not None
    n, steps, H, E, dev = args.lanes, args.steps, args.hidden, args.epochs, "cuda:0"
    gamma, lam, lr_pi, lr_v = 0.97, 0.9, 0.02, 0.01
    rng = np.random.default_rng(args.seed)
    policy = (0.1 * rng.standard_normal(gymrs.policy_size(gymrs.CARTPOLE, 0))).astype(np.float32)  # W[2][4], b[2]
    critic = (0.1 * rng.standard_normal(gymrs.critic_size(gymrs.CARTPOLE, H))).astype(np.float32)  # W1[H][4], b1[H], W2[H], b2

    params = gymrs.engine.default_params(gymrs.CARTPOLE)
    params.max_episode_steps = args.limit
    stream = torch.cuda.Stream()
    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT, params=params)
    env.set_stream(stream.cuda_stream)  # the engine launches on torch's stream
    env.reset(seed=args.seed)
    env.set_policy(policy, hidden=0, lanes_per_policy=n)
    env.set_critic(critic, hidden=H, lanes_per_critic=n)
    env.set_sampling(4321, temperature=1.0)

    stride = (n + 15) // 16 * 16
    grad_scale = 2.0**-24 / (steps * n)  # the table holds sums over K * n lane-steps in units of 2^-24
    with torch.cuda.stream(stream):
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        obs, final, start, rew = f32(steps, 4, stride), f32(steps, 4, stride), f32(4, stride), f32(steps, stride)
        act, done, trunc = u8(steps, stride), u8(steps, stride), u8(steps, stride)
        adv, ret, val = f32(steps, stride), f32(steps, stride), f32(steps, stride)
        norm_adv, zero, old_prob = f32(steps, stride), f32(steps, stride), f32(steps, stride)
        adv_stats = torch.zeros(5, dtype=torch.int64, device=dev)  # one gymrs_advantage_stats
        v_now = f32(steps, stride)  # V under the current critic: with this row given, value_gradient never allocates or synchronises
        g_pi, g_v = (torch.zeros((1, t.size), dtype=torch.int64, device=dev) for t in (policy, critic))
        x_pi, x_v, skipped = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(3))
        counts = torch.zeros((E, 1, 2), dtype=torch.int64, device=dev)  # a row per epoch
        ent_sums, ent_counts = (torch.zeros((E, 1, 2), dtype=torch.int64, device=dev) for _ in range(2))  # entropy and KL: a row per epoch too
        v_sums, v_counts = (torch.zeros((E, 1, 2), dtype=torch.int64, device=dev) for _ in range(2))  # squared errors, lane-steps seen and cut
        value_clip = dict(old_values=val.data_ptr(), clip=args.clip_vf) if args.clip_vf is not None else {}
        record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                      lane_stride=stride)
        rows = dict(record=record, start_obs=start.data_ptr())

        for r in range(args.rounds):
            env.rollout_transitions(steps, final_obs=final.data_ptr(), sample=True, **rows)
            env.advantages(steps, final_obs=final.data_ptr(), advantages=adv.data_ptr(), returns=ret.data_ptr(), values=val.data_ptr(), gamma=gamma,
                           lam=lam, critic=True, **rows)
            # old_prob: the prob row of the weights the record was drawn from (a zero coefficient row: the tables stay zero)
            env.policy_gradient(steps, coef=zero.data_ptr(), grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(), prob=old_prob.data_ptr(), temperature=1.0, **rows)
            env.normalize_advantages(steps, adv=adv.data_ptr(), out=norm_adv.data_ptr(), stats=adv_stats.data_ptr(), lane_stride=stride, lanes_per_policy=n)
            counts.zero_()
            v_sums.zero_()
            v_counts.zero_()
            ent_sums.zero_()
            ent_counts.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for e in range(E):  # nothing in here waits for the device
                env.ppo_gradient(steps, advantages=norm_adv.data_ptr(), old_prob=old_prob.data_ptr(), grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(),
                                 counts=counts[e].data_ptr(), clip=args.clip, temperature=1.0, **rows)
                if with_entropy:  # the bonus goes into the same table: the one apply_gradient below ascends the sum of both
                    env.entropy_gradient(steps, old_prob=old_prob.data_ptr(), grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(), sums=ent_sums[e].data_ptr(),
                                         counts=ent_counts[e].data_ptr(), coef=args.entropy, temperature=1.0, **rows)
                env.value_gradient(steps, returns=ret.data_ptr(), grad=g_v.data_ptr(), excluded=x_v.data_ptr(), sums=v_sums[e].data_ptr(),
                                   counts=v_counts[e].data_ptr(), values=v_now.data_ptr(), **value_clip, **rows)  # d/d phi of 0.5 * sum (V - R)^2, V computed in the kernel
                env.apply_gradient(grad=g_pi.data_ptr(), excluded=x_pi.data_ptr(), skipped=skipped.data_ptr(), adam=True, lr=lr_pi, grad_scale=grad_scale,
                                   ascend=True, zero_grad=True)  # ascend the clipped objective
                env.apply_gradient(grad=g_v.data_ptr(), excluded=x_v.data_ptr(), skipped=skipped.data_ptr(), critic=True, adam=True, lr=lr_v,
                                   grad_scale=grad_scale, max_norm=10.0, zero_grad=True)
            torch.cuda.synchronize()
            epoch_ms = (time.perf_counter() - t0) * 1e3 / max(1, E)

            fractions = [int(c[0, 1]) / max(1, int(c[0, 0])) for c in counts.cpu()]
            ends = int(((done | trunc) != 0)[:, :n].sum())
            env.rollout_closed_loop(steps, fitness=True)  # greedy validation with the new weights
            reward_sum, episodes, _, _ = env.policy_fitness()[0]
            env.policy_fitness_clear()
            print(f"round {r:2d}: {steps * n} sampled transitions, {ends} episode ends, clip fraction per epoch "
                  f"{' '.join(f'{f:.3f}' for f in fractions)}, {int(skipped[0])} updates skipped so far, {epoch_ms:.3f} ms per epoch; greedy validation: "
                  f"{int(reward_sum) / max(1, int(episodes) + n):.1f} steps per episode")
            vs, vc = v_sums.cpu().numpy()[:, 0], v_counts.cpu().numpy()[:, 0]
            print(f"          value loss per epoch {' '.join(f'{v:.4f}' for v in 0.5 * vs[:, 1] * 2.0**-24 / np.maximum(1, vc[:, 0]))}"
                  + (f", value clip fraction per epoch {' '.join(f'{v:.3f}' for v in vc[:, 1] / np.maximum(1, vc[:, 0]))}" if value_clip else ""))
            if with_entropy:  # read once per round, like counts
                s, c = ent_sums.cpu().numpy()[:, 0], ent_counts.cpu().numpy()[:, 0]
                entropy, kl = (s[:, j] * 2.0**-24 / np.maximum(1, c[:, j]) for j in (0, 1))
                beyond = [e for e in range(E) if args.target_kl is not None and kl[e] > args.target_kl]
                print(f"          entropy per epoch {' '.join(f'{v:.4f}' for v in entropy)}, KL estimate per epoch {' '.join(f'{v:.5f}' for v in kl)}"
                      + (f", beyond the target from epoch {beyond[0]}" if beyond else ""))
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
