#!/usr/bin/env python3
"""Long runs of the sequence test outside the suite: the generator of tests/sequence_ref.py with a free seed, every sequence
replayed on the device and on the CPU model and compared after every call (tests/sequence_replay.py).

    python tools/fuzz_sequences.py --cases 200 --seed 7

A mismatch prints the configuration, the calls up to the failing one and the first differing lanes, and exits 1; the sequence is
data and can be pasted into FIXED of tests/test_gpu_sequences.py to be shortened there.  Sequences that are not worth comparing
with (sequence_ref.worth_comparing: no episode ended, one action only, ..) are run all the same and counted."""
import argparse
import importlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime instance)

    gymrs = importlib.import_module("gym-rs_amd")
    import sequence_ref as sq
    import sequence_replay

    totals = {"cases": 0, "ops": 0, "steps": 0, "thin": 0}
    for k, (c, ops) in enumerate(sq.generate(args.seed, args.cases)):
        thin = sq.worth_comparing(c, ops)
        try:
            sequence_replay.replay(gymrs, c, ops)
        except sequence_replay.Mismatch as e:
            print(e)
            print(f"sequence {k} of seed {args.seed}: ({tuple(c)!r}, {ops!r})")
            return 1
        totals["cases"] += 1
        totals["ops"] += len(ops)
        totals["steps"] += sum(sq.steps_of(op) for op in ops)
        totals["thin"] += bool(thin)
        if args.verbose:
            print(sq.sequence_id(k, c), "ok", "; ".join(thin), flush=True)
    print("fuzz ok:", totals)
    return 0


if __name__ == "__main__":
    sys.exit(main())
