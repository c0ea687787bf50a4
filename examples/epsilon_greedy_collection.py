#!/usr/bin/env python
"""A Double-DQN style learner that never leaves the device: explore inside the fused launch, take the Q-gradient inside the library,
update the weights in place, refresh the target set every few rounds, validate greedily.

A linear Q-function on CartPole, Q(s, a) = W[a] . s + b[a], IS an affine policy of the engine (its argmax is the greedy action), so
the engine plays it inside the kernel and differentiates it inside the kernel.  Every round
  1. collects K whole transitions of every lane in ONE launch with `rollout_transitions(K, explore=True, ...)`: the action of a step
     is random with probability epsilon (decaying round by round) and the argmax otherwise; `final_obs` keeps the observation an
     ended lane showed before its re-arm, so truncated steps are kept and bootstrapped from it;
  2. recovers which recorded actions were exploratory with `explore_draw` from (global lane id, tick) alone -- no extra trajectory
     row -- and checks on a few lanes that an explored action is the draw's random action;
  3. takes the Q-gradient with `q_gradient(K, double=True, ...)` right behind the collection, no synchronisation in between: TD
     errors against the engine-owned target set, the Huber clamp, exact fixed-point sums;
  4. descends it in place through `policy_weights_ptr` (one torch operation on the engine's weights: no round trip to the host);
  5. every `--sync-every` rounds copies the online set into the target set with `q_target_sync`;
  6. validates the new policy with a greedy launch (`fitness=True`, no `explore`): fewer episodes ended = longer balancing.

With `--replay CAPACITY` step 3 and 4 become prioritized experience replay (include/gymrs_amd.h, "Replay"): the round's record is
pushed into a ring of CAPACITY transitions in device memory (`replay_push`), and `--updates` times a minibatch of B = lanes transitions
is drawn in proportion to the priorities (`replay_sample`), differentiated with `q_gradient(1, record=batch, final_obs=batch obs)`,
re-prioritised from the TD errors it wrote (`replay_update`) and applied with `apply_gradient` -- all on the engine's stream.

    python examples/epsilon_greedy_collection.py [--lanes 4096] [--steps 64] [--rounds 12] [--replay 1048576 [--updates 8]]
"""
from __future__ import annotations

import argparse
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
gymrs = importlib.import_module("gym-rs_amd")


class DeviceArray:
    """`count` elements of `typestr` at a device address, for torch.as_tensor (zero-copy)"""

    def __init__(self, ptr, count, typestr="<f4"):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=64, help="K: steps per launch")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--epsilon", type=float, default=0.5, help="of the first round; halves every third round")
    ap.add_argument("--sync-every", type=int, default=3, help="rounds between two q_target_sync")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--replay", type=int, default=0, metavar="CAPACITY", help="learn from a prioritized replay store of this many transitions")
    ap.add_argument("--updates", type=int, default=8, help="minibatches per round with --replay")
    args = ap.parse_args()
    n, steps, dev = args.lanes, args.steps, "cuda:0"
    gamma, kappa, lr, explore_seed = 0.97, 1.0, 0.05, 1234
    rng = np.random.default_rng(args.seed)
    size = gymrs.policy_size(gymrs.CARTPOLE, 0)  # W[2][4], b[2]

    env = gymrs.BatchedEngine(gymrs.CARTPOLE, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS | gymrs.TIME_LIMIT)
    env.reset(seed=args.seed)
    env.set_policy((0.1 * rng.standard_normal(size)).astype(np.float32), hidden=0, lanes_per_policy=n)
    env.q_target_sync()
    weights = torch.as_tensor(DeviceArray(*env.policy_weights_ptr()), device=dev)  # the engine's own buffer

    stride = (n + 15) // 16 * 16
    obs, final = (torch.empty((steps, 4, stride), dtype=torch.float32, device=dev) for _ in range(2))
    start = torch.empty((4, stride), dtype=torch.float32, device=dev)
    rew, td = (torch.empty((steps, stride), dtype=torch.float32, device=dev) for _ in range(2))
    act, done, trunc = (torch.empty((steps, stride), dtype=torch.uint8, device=dev) for _ in range(3))
    grad, excluded, counts = (torch.zeros(shape, dtype=torch.int64, device=dev) for shape in ((1, size), (1,), (1, 2)))
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(),
                  lane_stride=stride)
    probe = np.arange(0, n, max(1, n // 32))[:32]  # the lanes whose explored mask is recomputed on the host
    if args.replay:
        cap = max((args.replay + 15) // 16 * 16, (steps * n + 15) // 16 * 16)
        ring = dict(s=torch.zeros((4, cap), device=dev), s_next=torch.zeros((4, cap), device=dev), action=torch.zeros(cap, dtype=torch.uint8, device=dev),
                    reward=torch.zeros(cap, device=dev), done=torch.zeros(cap, dtype=torch.uint8, device=dev),
                    priority=torch.zeros(cap, dtype=torch.int32, device=dev))
        store = gymrs.Replay(*(ring[k].data_ptr() for k in ("s", "s_next", "action", "reward", "done", "priority")), cap)
        b_obs, b_start = (torch.empty((4, stride), dtype=torch.float32, device=dev) for _ in range(2))
        b_rew, b_td = (torch.empty(stride, dtype=torch.float32, device=dev) for _ in range(2))
        b_act, b_done = (torch.empty(stride, dtype=torch.uint8, device=dev) for _ in range(2))
        b_idx, b_prio = (torch.empty(stride, dtype=torch.int32, device=dev) for _ in range(2))
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        batch = dict(obs=b_obs.data_ptr(), actions=b_act.data_ptr(), reward=b_rew.data_ptr(), done=b_done.data_ptr(), lane_stride=stride)
        draws = 0

    for r in range(args.rounds):
        epsilon = args.epsilon * 0.5 ** (r // 3)
        env.set_exploration(explore_seed, epsilon=epsilon)
        _, threshold = env.exploration()  # epsilon on the grid of 1 / 65536
        t0 = env.tick()[0]                # row k of the record is the step from tick t0 + k
        # collection and the Q-gradient, back to back on the engine's stream
        env.rollout_transitions(steps, record=record, final_obs=final.data_ptr(), start_obs=start.data_ptr(), explore=True)
        if args.replay:
            env.replay_push(store, steps, record=record, start_obs=start.data_ptr(), final_obs=final.data_ptr())  # fresh: the highest priority
            for _ in range(args.updates):
                env.replay_sample(store, n, seed=args.seed, draw=draws, batch=batch, start_obs=b_start.data_ptr(), idx=b_idx.data_ptr(),
                                  prio=b_prio.data_ptr(), total=total.data_ptr())
                env.q_gradient(1, record=batch, start_obs=b_start.data_ptr(), final_obs=b_obs.data_ptr(), td=b_td.data_ptr(), grad=grad.data_ptr(),
                               excluded=excluded.data_ptr(), counts=counts.data_ptr(), gamma=gamma, kappa=kappa, double=True)
                env.replay_update(store, n, idx=b_idx.data_ptr(), td=b_td.data_ptr(), alpha=0.6, eps=1e-3, cap=4.0)
                env.apply_gradient(grad=grad.data_ptr(), excluded=excluded.data_ptr(), lr=lr, grad_scale=2.0**-24 / n, zero_grad=True)
                draws += 1
        else:
            env.q_gradient(steps, record=record, start_obs=start.data_ptr(), final_obs=final.data_ptr(), td=td.data_ptr(), grad=grad.data_ptr(),
                           excluded=excluded.data_ptr(), counts=counts.data_ptr(), gamma=gamma, kappa=kappa, double=True)
        env.sync()  # torch works on its own stream from here

        # which recorded actions were exploratory: recomputed from (global lane id, tick)
        explored, random_action = gymrs.explore_draw(explore_seed, threshold, 2, probe[None, :], t0 + np.arange(steps)[:, None])
        taken = act[:, :n].cpu().numpy()[:, probe]
        assert np.array_equal(taken[explored], random_action[explored])  # an explored step took the draw's action

        # descend the Huber loss in place: grad is the exact fixed-point sum over all lane-steps, times 2^24
        seen, clamped = (int(v) for v in counts[0])
        if not args.replay:
            weights -= (lr / max(1, seen) * 2.0**-24) * grad[0].double().float()
        mean_td = float((b_td[:n] if args.replay else td[:, :n]).abs().mean())
        grad.zero_(), excluded.zero_(), counts.zero_()
        torch.cuda.synchronize()  # the engine reads the weights on its own stream
        if (r + 1) % args.sync_every == 0:
            env.q_target_sync()

        # greedy validation: the closed-loop call without `explore`
        env.policy_fitness_clear()
        env.rollout_closed_loop(steps, fitness=True)
        reward_sum, episodes, _, _ = env.policy_fitness()[0]
        print(f"round {r:2d}: epsilon {threshold / 65536:.4f} ({explored.mean():.1%} of {explored.size} probed steps explored), "
              f"mean |TD| {mean_td:.3f}, {clamped / max(1, seen):.1%} of {seen} lane-steps clamped, "
              f"{int((trunc[:, :n] != 0).sum())} truncated steps kept"
              + (f", store {store.count} of {store.capacity}, mass {int(total[0]) / 2.0**24:.0f} x 2^24" if args.replay else "") + "; "
              f"greedy validation: {int(episodes)} episodes ended in {steps} x {n} lane-steps "
              f"(mean length {steps * n / max(1, int(episodes)):.1f})")
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
