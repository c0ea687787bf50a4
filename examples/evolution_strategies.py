#!/usr/bin/env python
"""Evolution strategies on CartPole with the whole generation loop on the device.

A population of `--policies` small policies around ONE centre: `es_init` writes generation 0 on the device, and every generation is
`evaluate_policy` (whole episodes of every member, in one launch) followed by `es_step` (utilities from the evaluation records, the
gradient of the centre from the regenerated noise, Adam, and the next population) -- in stream order, with no copy to the host and no
synchronisation inside the loop.  What the centre itself earns is watched by a second, small engine on the SAME stream: per generation
its one policy is overwritten with the centre (device to device), played, and its record kept in a device row that is read once,
after the loop.

    python examples/evolution_strategies.py [--policies 4096] [--hidden 0] [--generations 30] [--sigma 0.1] [--lr 0.05] [--ranks]
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


class DeviceRow:
    """A zero-copy torch view of n elements at a device address"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=4096, help="population size (even)")
    ap.add_argument("--hidden", type=int, default=0)
    ap.add_argument("--episodes", type=int, default=4, help="episodes per member and generation")
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ranks", action="store_true", help="shape by centred ranks (es_ranks) instead of the z-score of the mean return")
    args = ap.parse_args()
    P, size = args.policies, gymrs.policy_size(gymrs.CARTPOLE, args.hidden)
    centre0 = (0.1 * np.random.default_rng(args.seed).standard_normal(size)).astype(np.float32)

    env = gymrs.BatchedEngine(gymrs.CARTPOLE, P, flags=gymrs.AUTO_RESET)
    env.es_init(centre0, n_policies=P, sigma=args.sigma, seed=args.seed, hidden=args.hidden)
    probe_lanes = 256
    probe = gymrs.BatchedEngine(gymrs.CARTPOLE, probe_lanes, flags=gymrs.AUTO_RESET)
    probe.set_stream(env.stream)  # one stream orders everything below
    probe.set_policy(centre0[None], hidden=args.hidden, lanes_per_policy=probe_lanes)
    probe.evaluate_policy(1, seed=0)  # (the record table appears at its first use)
    env.sync()

    stream = torch.cuda.ExternalStream(env.stream)
    centre = torch.as_tensor(DeviceRow(*env.es_centre_ptr(), "<f4"), device="cuda")
    probe_weights = torch.as_tensor(DeviceRow(*probe.policy_weights_ptr(), "<f4"), device="cuda")
    probe_record = torch.as_tensor(DeviceRow(probe.policy_eval_ptr()[0], 8, "<i8"), device="cuda")
    with torch.cuda.stream(stream):
        history = torch.zeros((args.generations, 8), dtype=torch.int64, device="cuda")
        ranks = torch.zeros(P, dtype=torch.float32, device="cuda") if args.ranks else None
        for gen in range(args.generations):  # nothing in this loop waits for the device
            probe_weights.copy_(centre)
            probe.evaluate_policy(1, seed=10_000 + gen)
            history[gen].copy_(probe_record)
            env.evaluate_policy(args.episodes, seed=gen * args.episodes)
            if ranks is not None:  # centred ranks instead of z-scores: evaluate, ranks, step, still without a host round trip
                env.es_ranks(ranks.data_ptr())
            env.es_step(adam=True, lr=args.lr, grad_scale=2.0**-24 / (P * args.sigma), max_norm=10.0,
                        utilities=None if ranks is None else ranks.data_ptr())
    env.sync()
    for gen, row in enumerate(history.cpu().numpy()):
        print(f"generation {gen}: mean return of the centre {row[0] / row[2]:.1f} over {row[2]} episodes")
    print(f"generations on the device: {env.es_state(centre=False)['generation']} (a random policy earns about 22, the limit is 500)")
    probe.close()
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
