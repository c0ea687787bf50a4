"""gymrs_optimizer_set (host only) against the plain numpy restatement of tests/optimizer_ref.py, bit for bit, over three consecutive
calls: the rule of include/gymrs_amd.h, "Optimizer", is defined to the bit, so there is no tolerance."""
import numpy as np
import optimizer_ref as ref
import pytest

GRAD_SCALE = 2.0**-24 / 4096


def table(rng, S, call):
    """q uniform in +-2^40 with 0, +-1 and +-2^62 planted (the big pair in the first call only: the later calls do not clip)"""
    q = rng.integers(-(1 << 40), (1 << 40) + 1, S, dtype=np.int64)
    q[:3] = (0, 1, -1)
    if call == 0:
        q[3:5] = (1 << 62, -(1 << 62))
    return q


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("S", [9, 114, 450])
@pytest.mark.parametrize("tau", [0.0, 0.25])
@pytest.mark.parametrize("max_norm", [np.inf, 1000.0])
@pytest.mark.parametrize("kind", [ref.SGD, ref.ADAM])
def test_set_equals_the_reference(gymrs, kind, max_norm, tau, S):
    rng = np.random.default_rng([kind, int(tau * 4), S])
    w, target = (rng.standard_normal(S).astype(np.float32) for _ in range(2))
    w[0] = -0.0  # under q = 0
    m, v, pw = np.zeros(S, np.float32), np.zeros(S, np.float32), np.ones(2, np.float32)
    want = dict(w=w[None], m=m[None], v=v[None], pw=pw[None], target=target[None])
    hyper = dict(kind=kind, lr=0.01, grad_scale=GRAD_SCALE, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=max_norm, tau=tau, ascend=kind == ref.ADAM)
    clipped = []
    for call in range(3):
        q = table(rng, S, call)
        want = ref.apply(q[None], np.zeros(1, np.uint64), *(want[k] for k in ("w", "m", "v", "pw", "target")), **hyper)
        clipped.append(bool(want["clipped"][0]))
        adam = dict(m=m, v=v, pw=pw) if kind == ref.ADAM else {}
        w, m_, v_, pw_, target_ = gymrs.optimizer_set(q, w, target=target if tau > 0 else None, **adam, **hyper)
        if kind == ref.ADAM:
            m, v, pw = m_, v_, pw_
        if tau > 0:
            target = target_
        for name, got in (("w", w), ("m", m), ("v", v), ("pw", pw), ("target", target)):
            assert np.array_equal(bits(got), bits(want[name][0])), (name, call, np.argwhere(bits(got) != bits(want[name][0]))[:4])
    assert clipped == ([True, False, False] if max_norm < np.inf else [False] * 3)  # both sides of the compare were met


@pytest.mark.parametrize("bad, cause", [(dict(lr=np.nan), "lr"), (dict(grad_scale=np.inf), "grad_scale"), (dict(eps=-1.0), "eps"), (dict(beta1=1.0), "beta1"),
                                        (dict(beta2=-0.1), "beta2"), (dict(max_norm=0.0), "max_norm"), (dict(tau=1.5), "tau"), (dict(flags=4), "flag"),
                                        (dict(kind=2), "kind"), (dict(kind=ref.ADAM), "m, v and pw"), (dict(tau=0.5), "target")])
def test_set_refusals(gymrs, bad, cause):
    args = dict(kind=ref.SGD, lr=0.1, grad_scale=1.0)
    args.update(bad)
    with pytest.raises(gymrs.GymrsError, match=cause):
        gymrs.optimizer_set(np.zeros(9, np.int64), np.zeros(9, np.float32), **args)
