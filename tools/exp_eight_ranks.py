#!/usr/bin/env python
"""Developer experiment (profiles/r05_eight_ranks.log): `bench.py --gpus 8 --oversubscribe --n-envs 32768 --path <shape>` (8 processes sharing ONE GPU, 16
queues); prints OK when the line's episode statistics are those of the CPU f32 twin of all 8 x 32768 lanes taken through bench.py's schedule after its seeded
reset (per call shape: one lead-in repetition, the K = 30 timed steps in 5 repetitions; the second shape first steps one repetition's length untimed), the
statistics otherwise.  argv[1] = per_step_visible (HIP launches only) | chain | both.  (Round 5's record predates the seeded reset: its wanted figures were
those of the calibration-pinned schedule of that time.)"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "8", "--oversubscribe", "--n-envs", "32768", "--cpu-seconds", "0", "--steps", "30", "--warmup", "10", "--no-probe",
       "--repetitions", "5", "--action-buffers", "8", "--path", sys.argv[1], "--full-out", f"/tmp/eight_{os.getpid()}.json"]
sys.path.insert(0, str(ROOT))
import importlib  # noqa: E402

import bench  # noqa: E402
from oracle.bindings import Twin, TwinEngine  # noqa: E402

gymrs = importlib.import_module("gym-rs_amd")
twin = TwinEngine(Twin(), 0, 8 * 32768, gymrs.engine.default_params(0), flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS, gid0=0)
ring = [twin.fill_actions(1, b) for b in range(8)]
twin.reset(0)
sizes = bench.repetition_sizes(30, 5)
calls = [bench.lead_in_steps(sizes), *sizes]
if sys.argv[1] == "both":
    calls += [sizes[0], bench.lead_in_steps(sizes), *sizes]
for k in calls:
    for t in range(k):
        twin.step(ring[t % 8])
WANT = tuple(float(x) for x in twin.stats()[1:3])  # (sum_length, n_episodes)
env = dict(os.environ, GYMRS_BENCH_PASSES="2", HSA_ENABLE_IPC_MODE_LEGACY="0")  # (pins the untimed calibration: the run is shorter)
res = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
try:
    line = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    full = json.loads(Path(line["full"]).read_text())
    ep = full["episodes"]
    if (ep["sum_length"], ep["n_episodes"]) == WANT:
        print("OK")
    else:
        key = "chain" if sys.argv[1] == "both" else sys.argv[1]
        subs = sorted({str(r["paths"][key]["submission"])[:12] + "/" + str(r["paths"][key]["handover"])[:12] for r in full["ranks"]})
        per_rank = [(r["rank"], r.get("episodes")) for r in full["ranks"]]
        print(f"WRONG sum_length {ep['sum_length']:.0f} n_episodes {ep['n_episodes']:.0f} (want {WANT[0]:.0f} {WANT[1]:.0f}); submissions {subs}; per rank {per_rank}")
except Exception as exc:  # noqa: BLE001
    print("FAILED", res.returncode, repr(exc), res.stderr[-300:].replace("\n", " | "))
