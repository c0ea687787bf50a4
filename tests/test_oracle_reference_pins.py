"""Pins the oracle (and the product's host-side mirrors) against the reference's OWN unit tests —
the only tests the reference has for this path:
  src/spaces/discrete.rs:22-42        Discrete::contains
  src/utils/custom/util_fns.rs:12-33  clip
  src/utils/seeding.rs:28-40 + doctest :11-20   seed echo
The expected values live in tests/golden/reference_unit_tests.json (data copied from those tests)."""
import math


def test_discrete_contains_like_reference(golden, oracle, gymrs):
    for case in golden("reference_unit_tests")["discrete_contains"]:
        # given_value_greater_or_eq_than_upper_bound... / given_value_less_than_upper_bound...
        assert bool(oracle.lib.orc_discrete_contains(case["n"], case["value"])) is case["expect"]
        assert gymrs.Discrete(case["n"]).contains(case["value"]) is case["expect"]
        assert bool(gymrs.load_library().gymrs_discrete_contains(case["n"], case["value"])) is case["expect"]


def test_clip_like_reference(golden, oracle, twin):
    for case in golden("reference_unit_tests")["clip"]:
        v, l, r, want = case["value"], case["left"], case["right"], case["expect"]
        assert oracle.lib.orc_clip_i64(v, l, r) == want  # the reference tests clip on integers
        assert oracle.lib.orc_clip(float(v), float(l), float(r)) == float(want)
        assert twin.lib.twin_clipf(float(v), float(l), float(r)) == float(want)


def test_clip_total_order_nan(oracle, twin):
    # O64 = OrderedFloat<f64>: NaN is greater than every number, so clip(NaN, l, r) = r
    assert oracle.lib.orc_clip(math.nan, -1.0, 2.0) == 2.0
    assert twin.lib.twin_clipf(math.nan, -1.0, 2.0) == 2.0
    assert oracle.lib.orc_clip(-math.inf, -1.0, 2.0) == -1.0
    assert twin.lib.twin_clipf(math.inf, -1.0, 2.0) == 2.0


def test_seed_echo_like_reference(golden, oracle):
    # given_seed_when_rand_random_then_generator_is_created_using_seed (seeding.rs:33-39)
    for case in golden("reference_unit_tests")["seed_echo"]:
        assert oracle.lib.orc_rand_random_seed(1, case["seed"], 0xABCDEF) == case["expect"]
    assert oracle.lib.orc_rand_random_seed(0, 42, 0xABCDEF) == 0xABCDEF


def _reference_fixtures():
    """tests/golden/from_reference/*.json: written by bindings/rust/src/bin/make_golden.rs, i.e. by the reference's own
    step()/reset() on the inputs of tests/golden/*.json.  Absent in this repository's build image (no cargo/rustc)."""
    import json
    from pathlib import Path

    d = Path(__file__).resolve().parent / "golden" / "from_reference"
    if not (d / "cartpole.json").exists():
        return None
    return {n: json.loads((d / f"{n}.json").read_text()) for n in ("cartpole", "mountain_car")}


def test_oracle_against_fixtures_generated_by_the_reference(oracle):
    """The one-command pin of the oracle's physics by the reference itself:
        (cd bindings/rust && cargo run --release --bin make_golden) && python -m pytest tests/test_oracle_reference_pins.py
    Until someone with a Rust toolchain runs that, parity of step() stays "unpinned by the reference" (DESIGN.md §6)."""
    import numpy as np
    import pytest

    from oracle.bindings import CartPoleEnv, MountainCarEnv

    fx = _reference_fixtures()
    if fx is None:
        pytest.skip("tests/golden/from_reference/ not generated: this image has no cargo (bindings/rust/src/bin/make_golden.rs)")

    def ulps(a, b):
        return 0.0 if a == b else abs(a - b) / np.spacing(max(abs(a), abs(b)))

    p_other = oracle.cartpole_params()
    p_other.kinematics_integrator = 1
    for key, params in (("single_steps", None), ("semi_implicit", p_other)):
        for case in fx["cartpole"][key]:
            e = CartPoleEnv(*case["state"], 0, 0)
            rc, r = oracle.cartpole_step(e, case["action"], params)
            assert rc == 0 and r.reward == case["reward"] and bool(r.done) is case["done"]
            assert all(ulps(g, w) <= 2 for g, w in zip(r.obs, case["next"])), case  # libm pow(x, 2.0) vs x * x
    policies = {"always_1": lambda t: 1, "always_0": lambda t: 0, "alternate_1_0": lambda t: (t + 1) % 2}
    for tr in fx["cartpole"]["trajectories"]:
        e = CartPoleEnv(*tr["start"], 0, 0)
        t = 0
        while True:
            _, r = oracle.cartpole_step(e, policies[tr["policy"]](t))
            t += 1
            if r.done:
                break
        assert t == tr["steps"] and list(r.obs) == pytest.approx(tr["final"], rel=1e-9)
    bt = fx["cartpole"]["beyond_terminated"]
    e = CartPoleEnv(*bt["start"], 0, 0)
    got = [oracle.cartpole_step(e, bt["action"])[1] for _ in bt["rewards"]]
    assert [g.reward for g in got] == bt["rewards"] and [bool(g.done) for g in got] == bt["dones"]
    for case in fx["mountain_car"]["single_steps"]:
        e = MountainCarEnv(*case["state"])
        rc, r = oracle.mountain_car_step(e, case["action"])
        assert rc == 0 and r.reward == case["reward"] and bool(r.done) is case["done"]
        assert all(ulps(g, w) <= 1 for g, w in zip(list(r.obs)[:2], case["next"])), case
    for tr in fx["mountain_car"]["trajectories"]:
        e = MountainCarEnv(*tr["start"])
        t = 0
        while True:
            _, r = oracle.mountain_car_step(e, 2 if e.velocity >= 0 else 0)
            t += 1
            if r.done:
                break
        assert t == tr["steps"]


def test_default_constants_against_the_reference_source_text(oracle, golden, gymrs):
    """The default values of CartPoleEnv::new / MountainCarEnv::new (cartpole.rs:94-103, mountain_car.rs:344-351), the default reset
    boxes (cartpole.rs:353-360, mountain_car.rs:175-186) and the action-space sizes, read as numbers from the reference's source text into
    tests/golden/reference_constants.json, against the oracle's and the product's defaults.  No reference code is executed or copied."""
    import ctypes as C

    fx = golden("reference_constants")
    cp, mc = fx["cartpole"], fx["mountain_car"]
    p = oracle.cartpole_params()
    for name, want in cp["defaults"].items():
        assert getattr(p, name) == want, name
    q = oracle.mountain_car_params()
    for name, want in mc["defaults"].items():
        assert getattr(q, name) == want, name
    assert set(cp["defaults"]) == {"gravity", "masscart", "masspole", "length", "force_mag", "tau", "theta_threshold_radians", "x_threshold"}
    assert set(mc["defaults"]) == {"min_position", "max_position", "max_speed", "goal_position", "goal_velocity", "force", "gravity"}
    n = C.c_uint32()
    lib = gymrs.load_library()
    assert lib.gymrs_action_space(0, C.byref(n), None, None) == 0 and n.value == cp["action_space_n"] == 2
    assert lib.gymrs_action_space(1, C.byref(n), None, None) == 0 and n.value == mc["action_space_n"] == 3
    # default reset boxes: +-0.05 on every CartPole component, position in [-0.6, -0.4) for MountainCar
    assert cp["reset_low"] == [-0.05] * 4 and cp["reset_high"] == [0.05] * 4
    assert all(cp["reset_low"][j] <= v < cp["reset_high"][j] for j, v in enumerate(oracle.reset_pcg64(0, 1)))
    assert mc["reset_position_low"] <= oracle.reset_pcg64(1, 1)[0] < mc["reset_position_high"]
    # the quirk the build keeps: polemass_length = masspole + length (0.6), not Gym's product (0.05)
    assert cp["polemass_length"] == p.masspole + p.length and cp["polemass_length"] != p.masspole * p.length
