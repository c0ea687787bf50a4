"""The refusals of the learner surface of the C ABI (policy and critic sets, exploration and sampling, advantages, gradients, the
clipped surrogate, the host-only lanes, the fitness and evaluation tables), word for word.

The test_refusals of the per-feature GPU tests match substrings; this one pins the exact (status, gymrs_last_error()) of a fixed list of
bad calls, among them calls with two defects at once (which refusal wins is part of the interface), against
tests/golden/learner_refusals.json.  The file is a transcript of the library as it was BEFORE the host side of these calls was
consolidated, so the test passes unchanged on both sides of that change.  `python tests/test_learner_refusals.py --record host|gpu`
rewrites the respective part of the file from the library in use (GYMRS_AMD_LIB chooses one).

The four CartPole and MountainCar engines (16 and 48 lanes) must give one and the same transcript, which the file holds once.

No call here gets as far as a launch on caller buffers: every descriptor with n_steps != 0 carries a defect, and the buffer addresses
all lie inside one zeroed device allocation anyway."""
import ctypes as C
import importlib
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
GOLDEN = Path(__file__).resolve().parent / "golden" / "learner_refusals.json"
CARTPOLE, MOUNTAIN_CAR, PENDULUM = 0, 1, 2
NAN, INF = float("nan"), float("inf")
ENGINES = [("cartpole", CARTPOLE, 16), ("cartpole", CARTPOLE, 48), ("mountain_car", MOUNTAIN_CAR, 16), ("mountain_car", MOUNTAIN_CAR, 48)]
N_STEPS = (0, 3)


def package():
    return importlib.import_module("gym-rs_amd")


class Transcript:
    """rows of [entry point, what is wrong with the call, status, message ("" for GYMRS_OK: the last error is then a stale one)]"""

    def __init__(self, lib):
        self.lib, self.rows = lib, []

    def __call__(self, name, what, *args):
        st = getattr(self.lib, name)(*args)
        self.rows.append([name, what, st, self.lib.gymrs_last_error().decode("utf-8") if st else ""])
        return st


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------
def host_transcript(lib):
    t = Transcript(lib)
    eng = package().engine
    n64 = C.c_uint64()
    for name in ("gymrs_policy_size", "gymrs_critic_size"):
        t(name, "n_floats NULL", CARTPOLE, 0, None)
        t(name, "Pendulum", PENDULUM, 0, C.byref(n64))
        t(name, "no env kind", 7, 0, C.byref(n64))
        t(name, "hidden 65", CARTPOLE, 65, C.byref(n64))
        t(name, "n_floats NULL + Pendulum", PENDULUM, 0, None)
        t(name, "Pendulum + hidden 65", PENDULUM, 65, C.byref(n64))
        t(name, "fine: hidden 64", MOUNTAIN_CAR, 64, C.byref(n64))

    w, x, v = (C.c_float * 512)(), (C.c_float * 8)(), C.c_float()
    name = "gymrs_critic_value"
    t(name, "weights NULL", CARTPOLE, 0, None, x, C.byref(v))
    t(name, "obs NULL", CARTPOLE, 0, w, None, C.byref(v))
    t(name, "v NULL", CARTPOLE, 0, w, x, None)
    t(name, "Pendulum", PENDULUM, 0, w, x, C.byref(v))
    t(name, "hidden 65", MOUNTAIN_CAR, 65, w, x, C.byref(v))
    t(name, "v NULL + Pendulum", PENDULUM, 0, w, x, None)
    t(name, "Pendulum + hidden 65", PENDULUM, 65, w, x, C.byref(v))
    t(name, "fine", MOUNTAIN_CAR, 3, w, x, C.byref(v))

    acts, coef, q, excl, prob = (C.c_uint8 * 2)(), (C.c_float * 2)(), (C.c_int64 * 512)(), C.c_uint64(), (C.c_float * 2)()
    name = "gymrs_gradient_lane"

    def lane(what, kind=CARTPOLE, hidden=0, flags=0, scale=1.0, weights=w, n_steps=2, xs=x, actions=acts, c=coef, out=q, excluded=C.byref(excl), p=None):
        t(name, what, kind, hidden, flags, scale, weights, n_steps, xs, actions, c, out, excluded, p)

    lane("Pendulum", kind=PENDULUM)
    lane("hidden 65", hidden=65)
    lane("flag bit 1", flags=2)
    lane("weights NULL", weights=None)
    lane("coef NULL", c=None)
    lane("q NULL", out=None)
    lane("excluded NULL", excluded=None)
    lane("x NULL", xs=None)
    lane("fine: x NULL, no steps", xs=None, n_steps=0)
    lane("actions NULL", actions=None)
    lane("fine: actions NULL, no steps", actions=None, n_steps=0)
    lane("fine: actions NULL, critic", actions=None, flags=1)
    lane("prob, critic", flags=1, p=prob)
    for s in (-1.0, NAN, INF):
        lane(f"scale {s}", scale=s)
    lane("fine: scale nan, critic", scale=NAN, flags=1)
    lane("Pendulum + hidden 65", kind=PENDULUM, hidden=65)
    lane("hidden 65 + flag bit 1", hidden=65, flags=2)
    lane("flag bit 1 + weights NULL", flags=3, weights=None)
    lane("q NULL + actions NULL", out=None, actions=None)
    lane("actions NULL + scale nan", actions=None, scale=NAN)
    lane("prob, critic + x NULL", flags=1, p=prob, xs=None)
    lane("fine", kind=MOUNTAIN_CAR, hidden=5, p=prob)

    adv, old, counts = (C.c_float * 2)(), (C.c_float * 2)(0.5, 0.5), (C.c_uint64 * 2)()
    name = "gymrs_ppo_lane"

    def ppo(what, kind=CARTPOLE, hidden=0, scale=1.0, low=0.8, high=1.2, weights=w, n_steps=2, xs=x, actions=acts, a=adv, old_prob=old, out=q,
            excluded=C.byref(excl), cnt=counts, p=None):
        t(name, what, kind, hidden, scale, low, high, weights, n_steps, xs, actions, a, old_prob, out, excluded, cnt, p)

    ppo("Pendulum", kind=PENDULUM)
    ppo("hidden 65", hidden=65)
    for field, shown in (("weights", "weights"), ("a", "advantages"), ("old_prob", "old_prob"), ("out", "q"), ("excluded", "excluded"), ("xs", "x"),
                         ("actions", "actions")):
        ppo(f"{shown} NULL", **{field: None})
    ppo("fine: x and actions NULL, no steps", xs=None, actions=None, n_steps=0)
    ppo("prob is old_prob", p=old)
    for s in (-1.0, NAN, INF):
        ppo(f"scale {s}", scale=s)
    for low, high in ((-0.1, 1.2), (1.1, 1.2), (0.8, 0.9), (0.8, INF), (NAN, 1.2), (0.8, NAN)):
        ppo(f"clip bounds {low} {high}", low=low, high=high)
    ppo("fine: clip bounds 0 1, counts NULL", low=0.0, high=1.0, cnt=None)
    ppo("Pendulum + hidden 65", kind=PENDULUM, hidden=65)
    ppo("hidden 65 + weights NULL", hidden=65, weights=None)
    ppo("q NULL + prob is old_prob", out=None, p=old)
    ppo("prob is old_prob + scale nan", p=old, scale=NAN)
    ppo("scale -1 + clip bounds 2 2", scale=-1.0, low=2.0, high=2.0)
    ppo("fine", kind=MOUNTAIN_CAR, hidden=5, p=prob)

    u8 = C.c_uint8()
    name = "gymrs_explore_draw"
    t(name, "settings NULL", None, 2, 0, 0, C.byref(u8), C.byref(u8))
    t(name, "threshold 65537", C.byref(eng.Exploration(1, 65537, 0)), 2, 0, 0, C.byref(u8), C.byref(u8))
    t(name, "reserved 1", C.byref(eng.Exploration(1, 100, 1)), 2, 0, 0, C.byref(u8), C.byref(u8))
    t(name, "no actions", C.byref(eng.Exploration(1, 100, 0)), 0, 0, 0, C.byref(u8), C.byref(u8))
    t(name, "257 actions", C.byref(eng.Exploration(1, 100, 0)), 257, 0, 0, C.byref(u8), C.byref(u8))
    t(name, "threshold 65537 + reserved 1", C.byref(eng.Exploration(1, 65537, 1)), 2, 0, 0, C.byref(u8), C.byref(u8))
    t(name, "reserved 1 + no actions", C.byref(eng.Exploration(1, 100, 1)), 0, 0, 0, C.byref(u8), C.byref(u8))
    t(name, "fine: threshold 65536, 256 actions, no outputs", C.byref(eng.Exploration(1, 65536, 0)), 256, 5, 9, None, None)

    logits, act = (C.c_float * 8)(), C.c_uint8()
    name = "gymrs_sample_draw"
    t(name, "settings NULL", None, 2, logits, 0, 0, C.byref(act), prob)
    for s in (-1.0, NAN, INF):
        t(name, f"scale {s}", C.byref(eng.Sampling(1, s, 0)), 2, logits, 0, 0, C.byref(act), prob)
    t(name, "reserved 1", C.byref(eng.Sampling(1, 1.0, 1)), 2, logits, 0, 0, C.byref(act), prob)
    t(name, "1 action", C.byref(eng.Sampling(1, 1.0, 0)), 1, logits, 0, 0, C.byref(act), prob)
    t(name, "9 actions", C.byref(eng.Sampling(1, 1.0, 0)), 9, logits, 0, 0, C.byref(act), prob)
    t(name, "logits NULL", C.byref(eng.Sampling(1, 1.0, 0)), 2, None, 0, 0, C.byref(act), prob)
    t(name, "scale nan + reserved 1", C.byref(eng.Sampling(1, NAN, 1)), 2, logits, 0, 0, C.byref(act), prob)
    t(name, "reserved 1 + 9 actions", C.byref(eng.Sampling(1, 1.0, 1)), 9, logits, 0, 0, C.byref(act), prob)
    t(name, "9 actions + logits NULL", C.byref(eng.Sampling(1, 1.0, 0)), 9, None, 0, 0, C.byref(act), prob)
    t(name, "fine: scale 0, 8 actions, no outputs", C.byref(eng.Sampling(1, 0.0, 0)), 8, logits, 5, 9, None, None)

    # a NULL engine, with the other arguments in order and with every pointer NULL
    some = C.byref((C.c_uint8 * 256)())  # (stands for a descriptor or an output: never read, the engine is looked at first)
    p, n32 = C.c_void_p(), C.c_uint32()
    for name, rest in (("gymrs_set_policy", (some, some)), ("gymrs_get_policy", (some, some, 256)), ("gymrs_policy_weights_ptr", (C.byref(p), C.byref(n64))),
                       ("gymrs_policy_actions", (some,)), ("gymrs_set_exploration", (some,)), ("gymrs_get_exploration", (some,)),
                       ("gymrs_explore_actions", (some,)), ("gymrs_set_sampling", (some,)), ("gymrs_get_sampling", (some,)),
                       ("gymrs_sample_actions", (some, some)), ("gymrs_set_critic", (some, some)), ("gymrs_get_critic", (some, some, 256)),
                       ("gymrs_critic_weights_ptr", (C.byref(p), C.byref(n64))), ("gymrs_advantages", (some,)), ("gymrs_policy_gradient", (some,)),
                       ("gymrs_ppo_gradient", (some,)), ("gymrs_policy_fitness_ptr", (C.byref(p), C.byref(n32))), ("gymrs_get_policy_fitness", (0, 1, some)),
                       ("gymrs_policy_fitness_clear", ()), ("gymrs_evaluate_policy", (some,)), ("gymrs_policy_eval_ptr", (C.byref(p), C.byref(n32))),
                       ("gymrs_get_policy_eval", (0, 1, some))):
        t(name, "engine NULL", None, *rest)
        if rest:
            t(name, "engine NULL + the rest NULL or 0", None, *[0 if isinstance(a, int) else None for a in rest])
    return t.rows


# ---- with a GPU ----------------------------------------------------------------------------------------------------------------------
def _desc(cls, defaults, n_steps, change):
    """cls(n_steps, **defaults) with `change` applied; the keys "record.<field>" reach into the record"""
    fields = dict(defaults, n_steps=n_steps)
    record = dict(fields.pop("record"))
    for k, val in change.items():
        if k.startswith("record."):
            record[k[7:]] = val
        else:
            fields[k] = val
    return cls(record=package().engine.Trajectory(**record), **fields)


def record_calls(t, h, base, stride, n_steps, sets):
    """gymrs_advantages, gymrs_policy_gradient and gymrs_ppo_gradient on an engine whose kind and sets let a descriptor without a defect
    through (`fine`: run it too, where n_steps == 0 makes it return before the launch)"""
    eng = package().engine
    rec = dict(obs=base, actions=base, reward=base, done=base, truncated=base, lane_stride=stride)
    odd16, odd8 = base + 8, base + 4  # not 16-byte aligned (still 8-byte aligned), not 8-byte aligned
    fine = sets and n_steps == 0

    def wanted(what):  # without the sets: what the missing sets decide and a few calls around it; with them: everything else
        if sets:
            return "without a critic" not in what and what != "nothing wrong"
        return "without a critic" in what or what in ("reserved 1", "scale nan", "record.obs NULL", "nothing wrong")

    strides = (("lane_stride 0", 0), ("lane_stride n - 1", stride - 1 if stride > 16 else 15), ("lane_stride no multiple of 16", stride + 8))

    name = "gymrs_advantages"
    dflt = dict(flags=0, gamma=0.5, lam=0.5, record=rec, final_obs=base, start_obs=base, advantages=base, returns=base, values=base, reserved=0)

    def adv(what, **change):
        if not wanted(what):
            return
        t(name, f"K={n_steps}: {what}", h, C.byref(_desc(eng.AdvantagesDesc, dflt, n_steps, change)))

    adv("reserved 1", reserved=1)
    adv("flag bit 1", flags=2)
    adv("CRITIC without a critic", flags=1)
    for g in (-0.5, 1.5, NAN):
        adv(f"gamma {g}", gamma=g)
        adv(f"lambda {g}", lam=g)
    for f in ("record.obs", "record.reward", "record.done", "start_obs", "advantages"):
        adv(f"{f} NULL", **{f: None})
    for f in ("record.obs", "record.reward", "record.done", "record.truncated", "final_obs", "start_obs", "advantages", "returns", "values"):
        adv(f"{f} misaligned", **{f: odd16})
    for what, s in strides:
        adv(what, **{"record.lane_stride": s})
    adv("reserved 1 + flag bit 1", reserved=1, flags=2)
    adv("flag bit 1 + CRITIC without a critic", flags=3)
    adv("CRITIC without a critic + gamma nan", flags=1, gamma=NAN)
    adv("gamma 1.5 + lambda 1.5", gamma=1.5, lam=1.5)
    adv("lambda nan + record.obs NULL", lam=NAN, **{"record.obs": None})
    adv("record.done NULL + start_obs NULL", **{"record.done": None, "start_obs": None})
    adv("advantages NULL + values misaligned", advantages=None, values=odd16)
    adv("returns misaligned + lane_stride 0", returns=odd16, **{"record.lane_stride": 0})
    adv("fine: truncated, final_obs, returns, values NULL" if fine else "truncated, final_obs, returns, values NULL", final_obs=None, returns=None,
        values=None, **{"record.truncated": None, "reserved": 0 if fine else 1})

    name = "gymrs_policy_gradient"
    dflt = dict(flags=0, scale=1.0, pad_=0, record=rec, start_obs=base, coef=base, prob=base, grad=base, excluded=base, reserved=0)

    def grad(what, **change):
        if not wanted(what):
            return
        t(name, f"K={n_steps}: {what}", h, C.byref(_desc(eng.GradientDesc, dflt, n_steps, change)))

    grad("nothing wrong")  # (refused without a policy only: wanted() drops it with one)
    grad("reserved 1", reserved=1)
    grad("pad_ 1", pad_=1)
    grad("flag bit 1", flags=2)
    grad("CRITIC without a critic", flags=1)
    for s in (-1.0, NAN, INF):
        grad(f"scale {s}", scale=s)
    for f in ("record.obs", "record.actions", "start_obs", "coef", "grad", "excluded"):
        grad(f"{f} NULL", **{f: None})
    for f in ("record.obs", "record.actions", "start_obs", "coef", "prob"):
        grad(f"{f} misaligned", **{f: odd16})
    for f in ("grad", "excluded"):
        grad(f"{f} misaligned", **{f: odd8})
    for what, s in strides:
        grad(what, **{"record.lane_stride": s})
    grad("pad_ 1 + flag bit 1", pad_=1, flags=2)
    grad("flag bit 1 + CRITIC without a critic", flags=3)
    grad("scale nan + record.obs NULL", scale=NAN, **{"record.obs": None})
    grad("record.actions NULL + coef NULL", coef=None, **{"record.actions": None})
    grad("excluded NULL + prob misaligned", excluded=None, prob=odd16)
    grad("coef misaligned + grad misaligned", coef=odd16, grad=odd8)
    grad("excluded misaligned + lane_stride 0", excluded=odd8, **{"record.lane_stride": 0})
    grad("fine: prob NULL, grad 8-byte aligned" if fine else "prob NULL, grad 8-byte aligned", prob=None, grad=odd16, reserved=0 if fine else 1)

    name = "gymrs_ppo_gradient"
    dflt = dict(flags=0, scale=1.0, clip_low=0.8, clip_high=1.2, pad_=0, record=rec, start_obs=base, advantages=base, old_prob=base, prob=base + 4096,
                grad=base, excluded=base, counts=base, reserved=0)

    def ppo(what, **change):
        if not wanted(what):
            return
        t(name, f"K={n_steps}: {what}", h, C.byref(_desc(eng.PpoDesc, dflt, n_steps, change)))

    ppo("nothing wrong")
    ppo("reserved 1", reserved=1)
    ppo("pad_ 1", pad_=1)
    ppo("flags 1", flags=1)
    for s in (-1.0, NAN, INF):
        ppo(f"scale {s}", scale=s)
    for low, high in ((-0.1, 1.2), (1.1, 1.2), (0.8, 0.9), (0.8, INF), (NAN, 1.2), (0.8, NAN)):
        ppo(f"clip bounds {low} {high}", clip_low=low, clip_high=high)
    for f in ("record.obs", "record.actions", "start_obs", "advantages", "old_prob", "grad", "excluded"):
        ppo(f"{f} NULL", **{f: None})
    ppo("prob is old_prob", prob=base)
    for f in ("record.obs", "record.actions", "start_obs", "advantages", "old_prob", "prob"):
        ppo(f"{f} misaligned", **{f: odd16})
    for f in ("grad", "excluded", "counts"):
        ppo(f"{f} misaligned", **{f: odd8})
    for what, s in strides:
        ppo(what, **{"record.lane_stride": s})
    ppo("pad_ 1 + flags 1", pad_=1, flags=1)
    ppo("flags 1 + scale nan", flags=1, scale=NAN)
    ppo("scale -1 + clip bounds 2 2", scale=-1.0, clip_low=2.0, clip_high=2.0)
    ppo("clip bounds nan 1.2 + record.obs NULL", clip_low=NAN, **{"record.obs": None})
    ppo("old_prob NULL + prob NULL", old_prob=None, prob=None)
    ppo("excluded NULL + prob is old_prob", excluded=None, prob=base)
    ppo("prob is old_prob, both misaligned", prob=odd16, old_prob=odd16)
    ppo("old_prob misaligned + counts misaligned", old_prob=odd16, counts=odd8)
    ppo("grad misaligned + lane_stride 0", grad=odd8, **{"record.lane_stride": 0})
    ppo("fine: prob and counts NULL" if fine else "prob and counts NULL", prob=None, counts=None, reserved=0 if fine else 1)


def table_calls(t, h, host, n_policies):
    """the read-out calls of the fitness and the evaluation table"""
    p, n32 = C.c_void_p(), C.c_uint32()
    for kind in ("fitness", "eval"):
        ptr, get = f"gymrs_policy_{kind}_ptr", f"gymrs_get_policy_{kind}"
        t(ptr, "dev_out NULL", h, None, C.byref(n32))
        t(ptr, "n_policies NULL", h, C.byref(p), None)
        t(get, "host_out NULL", h, 0, 1, None)
        t(get, "one record beyond the set", h, n_policies, 1, host)
        t(get, "no records beyond the set", h, n_policies + 1, 0, host)
        t(get, "first + count = 2^32", h, 1, 2**32 - 1, host)
        t(get, "host_out NULL + one record beyond the set", h, n_policies, 1, None)
        t(get, "the whole set", h, 0, n_policies, host)
        t(get, "no records at the end of the set", h, n_policies, 0, host)
    t("gymrs_policy_fitness_clear", "", h)


def eval_calls(t, h, base):
    eng = package().engine
    name = "gymrs_evaluate_policy"

    def ev(what, episodes=1, max_steps=10, flags=0, reserved=0, lengths=None):
        t(name, what, h, C.byref(eng.EvalDesc(episodes, max_steps, 7, flags, reserved, lengths)))

    t(name, "desc NULL", h, None)
    ev("no episodes", episodes=0)
    ev("reserved 1", reserved=1)
    ev("flag bit 1", flags=2)
    ev("lengths_dev misaligned", lengths=base + 2)
    ev("2^24 + 1 steps", episodes=2**24 + 1, max_steps=1)
    ev("more than 2^24 steps under the params' limit", episodes=2**18, max_steps=0)
    ev("no episodes + reserved 1", episodes=0, reserved=1)
    ev("reserved 1 + flag bit 1", reserved=1, flags=2)
    ev("flag bit 1 + lengths_dev misaligned", flags=2, lengths=base + 2)
    ev("lengths_dev misaligned + 2^24 + 1 steps", lengths=base + 2, episodes=2**24 + 1, max_steps=1)


def discrete_transcript(engine, base):
    """every engine-taking call of the learner surface on a CartPole or MountainCar engine: without sets, with bad sets, with sets"""
    pkg = package()
    eng = pkg.engine
    t = Transcript(engine._lib)
    h, kind, n = engine._h, engine.kind, engine.n_envs
    stride = (n + 15) // 16 * 16
    host = (C.c_uint8 * 4096)()
    desc, p, n64 = eng.PolicyDesc(), C.c_void_p(), C.c_uint64()

    def set_calls(noun, state):
        get, ptr = f"gymrs_get_{noun}", f"gymrs_{noun}_weights_ptr"
        t(get, f"{state}: desc NULL", h, None, host, 1024)
        t(get, f"{state}: a query", h, C.byref(desc), None, 0)
        t(get, f"{state}: room for one float", h, C.byref(desc), host, 1)
        t(get, f"{state}: weights_out NULL", h, C.byref(desc), None, 1024)
        t(get, f"{state}: room", h, C.byref(desc), host, 1024)
        t(ptr, f"{state}: dev_out NULL", h, None, C.byref(n64))
        t(ptr, f"{state}: n_floats NULL", h, C.byref(p), None)

    def launches(state):
        t("gymrs_policy_actions", f"{state}: actions_dev NULL", h, None)
        t("gymrs_explore_actions", f"{state}: actions_dev NULL", h, None)
        t("gymrs_sample_actions", f"{state}: actions_dev NULL", h, None, base)
        t("gymrs_sample_actions", f"{state}: prob_dev misaligned", h, base, base + 2)

    # no policy, no critic, no settings
    set_calls("policy", "no policy")
    set_calls("critic", "no critic")
    launches("no policy")
    t("gymrs_policy_actions", "no policy", h, base)
    t("gymrs_explore_actions", "no policy, no settings", h, base)
    t("gymrs_sample_actions", "no policy, no settings", h, base, None)
    t("gymrs_get_exploration", "no settings", h, host)
    t("gymrs_get_exploration", "x_out NULL", h, None)
    t("gymrs_get_sampling", "no settings", h, host)
    t("gymrs_get_sampling", "x_out NULL", h, None)
    table_calls(t, h, host, 3)
    eval_calls(t, h, base)
    for name in ("gymrs_advantages", "gymrs_policy_gradient", "gymrs_ppo_gradient"):
        t(name, "desc NULL", h, None)
    for k in N_STEPS:
        record_calls(t, h, base, stride, k, sets=False)

    # the settings
    for name, cls, bad in (("gymrs_set_exploration", eng.Exploration, 65537), ("gymrs_set_sampling", eng.Sampling, NAN)):
        t(name, "a bad value", h, C.byref(cls(1, bad, 0)))
        t(name, "reserved 1", h, C.byref(cls(1, 1, 1)))
        t(name, "a bad value + reserved 1", h, C.byref(cls(1, bad, 1)))
    t("gymrs_set_sampling", "scale -1", h, C.byref(eng.Sampling(1, -1.0, 0)))
    t("gymrs_set_sampling", "scale inf", h, C.byref(eng.Sampling(1, INF, 0)))
    t("gymrs_get_exploration", "after refused settings", h, host)
    t("gymrs_get_sampling", "after refused settings", h, host)

    # the sets
    weights = (C.c_float * 4096)()
    for noun in ("policy", "critic"):
        name = f"gymrs_set_{noun}"
        t(name, "hidden 65", h, C.byref(eng.PolicyDesc(65, 3, 8)), weights)
        t(name, "no networks", h, C.byref(eng.PolicyDesc(0, 0, 8)), weights)
        t(name, "no lanes per network", h, C.byref(eng.PolicyDesc(0, 3, 0)), weights)
        t(name, "weights_host NULL", h, C.byref(eng.PolicyDesc(0, 3, 8)), None)
        t(name, "hidden 65 + no networks", h, C.byref(eng.PolicyDesc(65, 0, 8)), weights)
        t(name, "no networks + no lanes per network", h, C.byref(eng.PolicyDesc(0, 0, 0)), weights)
        t(name, "no lanes per network + weights_host NULL", h, C.byref(eng.PolicyDesc(0, 3, 0)), None)
        set_calls(noun, f"after a refused {noun}")
        t(name, "removing what is not there", h, None, None)
    t("gymrs_set_critic", "3 critics, hidden 5", h, C.byref(eng.PolicyDesc(5, 3, 8)), weights)
    set_calls("critic", "a critic")
    set_calls("policy", "a critic, no policy")
    for k in N_STEPS:  # a critic alone: the critic heads pass, the policy heads still have no policy
        t("gymrs_policy_gradient", f"K={k}: no policy", h, C.byref(_desc(eng.GradientDesc, dict(flags=0, scale=1.0, pad_=0, record=dict(
            obs=base, actions=base, reward=base, done=base, truncated=base, lane_stride=stride), start_obs=base, coef=base, prob=base, grad=base,
            excluded=base, reserved=0), k, {})))
    t("gymrs_set_policy", "3 policies, hidden 5", h, C.byref(eng.PolicyDesc(5, 3, 8)), weights)
    set_calls("policy", "a policy")
    launches("a policy")
    t("gymrs_explore_actions", "a policy, no settings", h, base)
    t("gymrs_sample_actions", "a policy, no settings", h, base, None)
    for noun, cls in (("exploration", eng.Exploration), ("sampling", eng.Sampling)):
        t(f"gymrs_set_{noun}", "fine", h, C.byref(cls(1, 1, 0)))
        t(f"gymrs_get_{noun}", "fine", h, host)
        t(f"gymrs_get_{noun}", "x_out NULL", h, None)
        launches(f"a policy, {noun}")
        t(f"gymrs_set_{noun}", "a bad value keeps the old ones", h, C.byref(cls(1, 65537 if noun == "exploration" else -1.0, 0)))
        t(f"gymrs_get_{noun}", "fine", h, host)
        t(f"gymrs_set_{noun}", "remove", h, None)
        t(f"gymrs_get_{noun}", "removed", h, host)
    table_calls(t, h, host, 3)
    eval_calls(t, h, base)
    rows = (eng.CartPoleParams if kind == CARTPOLE else eng.MountainCarParams) * 2
    t("gymrs_set_param_table", "two rows", h, rows(engine.params, engine.params), 2)
    t("gymrs_evaluate_policy", "a parameter table, no opt-in", h, C.byref(eng.EvalDesc(1, 10, 7, 0, 0, None)))
    t("gymrs_evaluate_policy", "a parameter table, no opt-in + no episodes", h, C.byref(eng.EvalDesc(0, 10, 7, 0, 0, None)))
    t("gymrs_evaluate_policy", "a parameter table, opt-in, no episodes", h, C.byref(eng.EvalDesc(0, 10, 7, eng.EVAL_LANE_PARAMS, 0, None)))
    t("gymrs_set_param_table", "off", h, None, 0)
    for k in N_STEPS:
        record_calls(t, h, base, stride, k, sets=True)
    critic = dict(flags=1, record=dict(obs=base, actions=None, reward=base, done=base, truncated=base, lane_stride=stride), start_obs=base, reserved=0)
    for k in N_STEPS:  # the critic heads' own rules
        adv = dict(critic, gamma=0.5, lam=0.5, final_obs=base, advantages=base, returns=base, values=base)
        t("gymrs_advantages", f"K={k}: CRITIC, gamma nan", h, C.byref(_desc(eng.AdvantagesDesc, adv, k, dict(gamma=NAN))))
        grad = dict(critic, scale=NAN, pad_=0, coef=base, prob=None, grad=base, excluded=base)
        t("gymrs_policy_gradient", f"K={k}: CRITIC, prob", h, C.byref(_desc(eng.GradientDesc, grad, k, dict(prob=base))))
        t("gymrs_policy_gradient", f"K={k}: CRITIC, excluded NULL + prob", h, C.byref(_desc(eng.GradientDesc, grad, k, dict(prob=base, excluded=None))))
        t("gymrs_policy_gradient", f"K={k}: CRITIC, prob + coef misaligned", h, C.byref(_desc(eng.GradientDesc, grad, k, dict(prob=base, coef=base + 8))))
        t("gymrs_policy_gradient", f"K={k}: CRITIC, start_obs misaligned", h, C.byref(_desc(eng.GradientDesc, grad, k, dict(start_obs=base + 8))))
    t("gymrs_advantages", "K=0: fine: CRITIC", h, C.byref(_desc(eng.AdvantagesDesc, adv, 0, {})))
    t("gymrs_policy_gradient", "K=0: fine: CRITIC, scale nan, record.actions NULL and misaligned", h, C.byref(_desc(eng.GradientDesc, grad, 0, {})))
    t("gymrs_policy_gradient", "K=0: fine: CRITIC, record.actions misaligned", h,
      C.byref(_desc(eng.GradientDesc, grad, 0, {"record.actions": base + 1})))

    # the sets again: a smaller one, then none
    t("gymrs_set_policy", "2 policies, affine", h, C.byref(eng.PolicyDesc(0, 2, 1)), weights)
    table_calls(t, h, host, 2)
    set_calls("policy", "a smaller policy")
    t("gymrs_set_policy", "a refused set keeps the old one", h, C.byref(eng.PolicyDesc(65, 2, 1)), weights)
    set_calls("policy", "after a refused set")
    for noun in ("policy", "critic"):
        t(f"gymrs_set_{noun}", "remove", h, None, weights)
        set_calls(noun, "removed")
    table_calls(t, h, host, 2)
    t("gymrs_sync", "", h)
    return t.rows


def pendulum_transcript(engine, base):
    """the Discrete-only refusals: every call of the learner surface that looks at the env kind, on a Pendulum engine"""
    eng = package().engine
    t = Transcript(engine._lib)
    h, stride = engine._h, (engine.n_envs + 15) // 16 * 16
    host, weights = (C.c_uint8 * 4096)(), (C.c_float * 4096)()
    p, n32, n64 = C.c_void_p(), C.c_uint32(), C.c_uint64()
    for noun in ("policy", "critic"):
        t(f"gymrs_set_{noun}", "a set", h, C.byref(eng.PolicyDesc(0, 3, 8)), weights)
        t(f"gymrs_set_{noun}", "a set + hidden 65", h, C.byref(eng.PolicyDesc(65, 3, 8)), weights)
        t(f"gymrs_set_{noun}", "remove", h, None, None)
        t(f"gymrs_get_{noun}", "", h, host, host, 1024)
        t(f"gymrs_{noun}_weights_ptr", "", h, C.byref(p), C.byref(n64))
    t("gymrs_policy_actions", "", h, base)
    for name, cls in (("gymrs_set_exploration", eng.Exploration), ("gymrs_set_sampling", eng.Sampling)):
        t(name, "settings", h, C.byref(cls(1, 1, 0)))
        t(name, "settings + reserved 1", h, C.byref(cls(1, 1, 1)))
        t(name, "remove", h, None)
    t("gymrs_get_exploration", "", h, host)
    t("gymrs_get_sampling", "", h, host)
    t("gymrs_explore_actions", "", h, base)
    t("gymrs_sample_actions", "", h, base, None)
    t("gymrs_policy_fitness_ptr", "", h, C.byref(p), C.byref(n32))
    t("gymrs_get_policy_fitness", "", h, 0, 1, host)
    t("gymrs_get_policy_fitness", "no records", h, 0, 0, host)
    t("gymrs_policy_fitness_clear", "", h)
    t("gymrs_policy_eval_ptr", "", h, C.byref(p), C.byref(n32))
    t("gymrs_get_policy_eval", "", h, 0, 1, host)
    t("gymrs_evaluate_policy", "", h, C.byref(eng.EvalDesc(1, 10, 7, 0, 0, None)))
    t("gymrs_evaluate_policy", "+ no episodes", h, C.byref(eng.EvalDesc(0, 10, 7, 0, 0, None)))
    rec = dict(obs=base, actions=base, reward=base, done=base, truncated=base, lane_stride=stride)
    for k in N_STEPS:
        for what, change in (("", {}), (" + reserved 1", dict(reserved=1)), (" + record.obs NULL", {"record.obs": None})):
            t("gymrs_advantages", f"K={k}:{what}", h, C.byref(_desc(eng.AdvantagesDesc, dict(
                flags=0, gamma=0.5, lam=0.5, record=rec, final_obs=base, start_obs=base, advantages=base, returns=base, values=base, reserved=0), k, change)))
            t("gymrs_policy_gradient", f"K={k}:{what}", h, C.byref(_desc(eng.GradientDesc, dict(
                flags=0, scale=1.0, pad_=0, record=rec, start_obs=base, coef=base, prob=base, grad=base, excluded=base, reserved=0), k, change)))
            t("gymrs_ppo_gradient", f"K={k}:{what}", h, C.byref(_desc(eng.PpoDesc, dict(
                flags=0, scale=1.0, clip_low=0.8, clip_high=1.2, pad_=0, record=rec, start_obs=base, advantages=base, old_prob=base, prob=base + 4096,
                grad=base, excluded=base, counts=base, reserved=0), k, change)))
    for name in ("gymrs_advantages", "gymrs_policy_gradient", "gymrs_ppo_gradient", "gymrs_evaluate_policy"):
        t(name, "desc NULL", h, None)
    t("gymrs_sync", "", h)
    return t.rows


def gpu_transcript():
    import torch

    pkg = package()
    scratch = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda:0")  # every device address of the calls lies in here
    torch.cuda.synchronize()
    out = {}
    for name, kind, n in ENGINES:  # no message names the env or depends on the lanes: the four transcripts are one
        with pkg.BatchedEngine(kind, n, flags=pkg.AUTO_RESET) as engine:
            engine.reset(seed=1)
            rows = discrete_transcript(engine, scratch.data_ptr())
            same(rows, out.setdefault("discrete", rows), f"{name}/{n} against {ENGINES[0][0]}/{ENGINES[0][2]}")
    with pkg.BatchedEngine(PENDULUM, 16, flags=pkg.AUTO_RESET) as engine:
        engine.reset(seed=1)
        out["pendulum"] = pendulum_transcript(engine, scratch.data_ptr())
    assert not scratch.any().item(), "a refused call wrote to a caller buffer"
    return out


def same(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, (where, len(bad), bad[:5])


def test_host_refusals_are_worded_as_before():
    same(host_transcript(package().load_library()), json.loads(GOLDEN.read_text())["host"], "host")


@pytest.mark.gpu
def test_engine_refusals_are_worded_as_before():
    want = json.loads(GOLDEN.read_text())["gpu"]
    got = gpu_transcript()
    assert sorted(got) == sorted(want)
    for key in want:
        same(got[key], want[key], key)


if __name__ == "__main__":
    part = sys.argv[sys.argv.index("--record") + 1]
    if part == "gpu":
        import torch  # noqa: F401  (first, so the extension shares torch's HIP runtime instance)
    doc = json.loads(GOLDEN.read_text()) if GOLDEN.exists() else {}
    doc[part] = host_transcript(package().load_library()) if part == "host" else gpu_transcript()
    rows = lambda v: "[\n" + ",\n".join(json.dumps(r) for r in v) + "\n]"  # noqa: E731  (one call per line)
    parts = {k: rows(v) if k == "host" else "{\n" + ",\n".join(f"{json.dumps(e)}: {rows(r)}" for e, r in sorted(v.items())) + "\n}" for k, v in doc.items()}
    GOLDEN.write_text("{\n" + ",\n".join(f"{json.dumps(k)}: {parts[k]}" for k in sorted(parts)) + "\n}\n")
    print(part, sum(len(v) for v in doc[part].values()) if part == "gpu" else len(doc[part]), "calls recorded")
