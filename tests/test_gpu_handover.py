"""The hand-over amplifier as a test (VERDICT r5 "next" #1a, #2): tools/handover_amp.py -- PROCS processes share the one GPU of the test box, each loops
{seeded reset -> 100 steps in four gymrs_step_many calls with a statistics read in between -> gymrs_stats_clear -> six calls of 60 steps -> statistics}
hundreds of times per second and compares EVERY iteration's four numbers with the CPU f32 twin's for its (rank, seed): reset, the statistics read-out and
the clear sit between the calls of every iteration, so each of them is crossed thousands of times per run.

Two runs: the DEFAULT submission (HIP launches on the engine's stream) and the opt-in chains (GYMRS_AQL=1: the engine's own HSA queue, where every call is
a hand-over pair stream -> chain -> stream).  A WRONG count is a failure on either.  A chain call that fails LOUDLY (the per-launch XCD check, GYMRS_EHIP) is
not: when more processes hold the GPU than it has hardware process slots (eight), the kernel driver time-slices whole processes, remaps their queues, and
a chain's workgroups can start on another XCD in mid-chain; the check exists to say so (profiles/r06_handover_amp_12_processes_*.log: ~1 loud failure per 10^5
chain calls with 12 processes, one in 2.3 M with 8; never a wrong count).  Round 6's soak of this tool: > 10^6 chain calls without a wrong count
(profiles/r06_handover_amp_*.log).

How many workers run: PROCS = GYMRS_TEST_GPU_PROCESSES - 1, at most 8 (the pytest process holds a HIP context of its own and counts).  The eight-worker form
the tests are named after holds the GPU in 9 processes; the GPU machines that run this suite from a clean checkout stop a run once more than 6 processes hold
the GPU (the suite's eight-rank bench test, 10 processes, was stopped there), so the default is 6: five workers.  GYMRS_TEST_GPU_PROCESSES=9 (or more) runs
the eight-worker form -- the regime beyond the GPU's eight hardware process slots that the loud-failure bound below was written for -- where a machine allows
it; a run of the smaller form says so with a warning."""
import json
import os
import spawn_server
import sys
import warnings
from pathlib import Path

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.oversubscribed]
ROOT = Path(__file__).resolve().parent.parent
GPU_PROCESSES = int(os.environ.get("GYMRS_TEST_GPU_PROCESSES", "6"))  # processes with the GPU open at once, this one included
PROCS = max(1, min(8, GPU_PROCESSES - 1))


def _say_which_form():
    if PROCS < 8:
        warnings.warn(f"hand-over amplifier with {PROCS} workers, not the eight-worker form (GYMRS_TEST_GPU_PROCESSES={GPU_PROCESSES}; the eight-worker form "
                      f"needs 9 processes with the GPU open)")


def amplify(*args):
    _say_which_form()
    out = spawn_server.run([sys.executable, "tools/handover_amp.py", "--procs", str(PROCS), "--seconds", "20", *args], cwd=ROOT, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert lines, out.stdout[-2000:] + out.stderr[-3000:]
    rec = json.loads(lines[-1])
    print(json.dumps({k: rec[k] for k in ("mode", "handover", "iterations", "chain_calls", "wrong_iterations", "loud_failures", "trips", "errors")}))
    return rec


def test_default_submission_under_eight_processes():
    rec = amplify("--mode", "hip", "--lockstep")
    assert rec["wrong_iterations"] == 0 and not rec["errors"] and rec["loud_failures"] == 0, rec["bad"] or rec["errors"] or rec["trips"]
    assert rec["iterations"] >= PROCS * 50  # (a few hundred iterations per second on an idle box: this only says the loop ran)


@pytest.mark.parametrize("mode", ["both", "chain"])
def test_opt_in_chains_under_eight_processes(mode):
    rec = amplify("--mode", mode, "--handover", "auto")
    assert rec["wrong_iterations"] == 0 and not rec["errors"], rec["bad"] or rec["errors"]
    assert rec["chain_calls"] >= PROCS * 100
    # loud failures are the product saying "this chain's premise did not hold" (see the docstring): reported, bounded, not silent
    assert rec["loud_failures"] <= rec["chain_calls"] // 1000 + 2, rec["trips"]


@pytest.mark.parametrize("mode", ["hip", "both"])
def test_every_hand_over_class_under_eight_processes(mode):
    """VERDICT r5 "next" #2: every stream-side writer whose output the next launches read, and every read-out right behind a call, per iteration -- seeded reset,
    statistics read, clear, the state read out and written back (gymrs_get_state / gymrs_set_state), snapshot + a discarded call + restore (gymrs_snapshot_load), a
    step-result read-out, and with GYMRS_TIME_LIMIT the refresh kernels and the `truncated` memset between launches -- with state bits, reward / done / truncated and
    the statistics against the twin every time."""
    rec = amplify("--mode", mode, "--audit", "--flags", "7")
    assert rec["wrong_iterations"] == 0 and not rec["errors"], rec["bad"] or rec["errors"]
    assert rec["iterations"] >= PROCS * 20
    assert rec["loud_failures"] <= rec["chain_calls"] // 1000 + 2, rec["trips"]
