"""include/gymrs_amd.h "V-trace" on the CPU: op for op in f32 numpy for one lane, and the f64 sums of Espeholt et al. 2018 (eq. 1, 4.2).  Never imports the library."""
import advantages_ref as adv
import gradient_ref as ref
import numpy as np
import sample_ref as sr
from closed_loop_ref import DIMS
from value_ref import fma32, forward64

F = np.float32


def record(kind, n, steps, seed, end_rows=()):
    """ends at 8 % of the lane-steps and, on every row of `end_rows`, a done on lanes 0, 4, .. and a truncated-only step on lanes 1, 5, ..; NaN-sentinel final_obs elsewhere"""
    d, a = DIMS[kind]
    rng = np.random.default_rng([seed, kind, n, steps])
    r = dict(kind=kind, n=n, steps=steps, obs=rng.standard_normal((steps, d, n)).astype(F), start_obs=rng.standard_normal((d, n)).astype(F),
             reward=rng.standard_normal((steps, n)).astype(F), actions=rng.integers(0, a, (steps, n)).astype(np.uint8),
             done=(rng.random((steps, n)) < 0.04).astype(np.uint8), truncated=(rng.random((steps, n)) < 0.04).astype(np.uint8))
    for k in end_rows:
        r["done"][k, 0::4], r["truncated"][k, 0::4], r["done"][k, 1::4], r["truncated"][k, 1::4] = 1, 0, 0, 1
    r["ended"] = ((r["done"] != 0) | (r["truncated"] != 0)).astype(np.uint8)
    final = np.full((steps, d, n), adv.SENTINEL, np.uint32).view(F)
    r["final_obs"] = np.where(r["ended"][:, None, :] != 0, rng.standard_normal((steps, d, n)).astype(F), final)
    return r


def lane_inputs(r, i, final=True):
    """(x [K][D], x_next [K][D], actions, reward, done, ended) of lane i as gymrs_vtrace_lane takes them"""
    x = np.concatenate([r["start_obs"][None, :, i], r["obs"][:-1, :, i]])
    x_next = np.where(r["ended"][:, None, i] != 0, r["final_obs"][:, :, i], r["obs"][:, :, i]) if final else r["obs"][:, :, i]
    return x, x_next, r["actions"][:, i], r["reward"][:, i], r["done"][:, i], r["ended"][:, i]


def lane32(kind, hp, hc, wp, wc, x, x_next, actions, reward, done, ended, old_prob, gamma, lam, scale, bars):
    """(vs, pg, values, prob, counts) of one lane: the header's text line for line, every operation one f32 operation"""
    k, n_act = len(reward), DIMS[kind][1]
    pa_row = ref.lane(kind, hp, False, scale, wp, x, actions, np.zeros(k, F), prob=True)[2]
    gamma, lam, (rho_bar, c_bar, pg_bar) = F(gamma), F(lam), (F(b) for b in bars)
    vs, pg, values, prob, counts, acc = np.zeros(k, F), np.zeros(k, F), np.zeros(k, F), np.zeros(k, F), [0, 0, 0], F(0.0)
    with np.errstate(all="ignore"):
        for j in range(k - 1, -1, -1):
            v_cur = adv.critic_value(kind, hc, wc, x[j])
            v_next = F(0.0) if done[j] else adv.critic_value(kind, hc, wc, x_next[j])
            valid = actions[j] < n_act
            ratio = F(pa_row[j]) / F(old_prob[j]) if valid else F(0.0)
            rho = rho_bar if ratio > rho_bar else ratio
            cc = lam * (c_bar if ratio > c_bar else ratio)
            rho_pg = pg_bar if ratio > pg_bar else ratio
            td = fma32(gamma, v_next, reward[j]) - v_cur
            carry = F(0.0) if ended[j] else acc
            gc = gamma * cc
            acc = fma32(gc, carry, rho * td)
            vs[j] = acc + v_cur
            vs_next = carry + v_next
            pg[j] = rho_pg * (fma32(gamma, vs_next, reward[j]) - v_cur)
            values[j], prob[j] = v_cur, pa_row[j] if valid else F(0.0)
            counts = [counts[0] + int(valid), counts[1] + int(valid and ratio > rho_bar), counts[2] + int(valid and ratio > c_bar)]
    return vs, pg, values, prob, counts


def prob64(kind, hidden, w, x, action, scale):
    """pi(action | x) of the softmax policy in f64"""
    d, a = DIMS[kind]
    w, x = np.asarray(w, np.float64), np.asarray(x, np.float64)
    if hidden == 0:
        y = w[a * d:] + w[:a * d].reshape(a, d) @ x
    else:
        z = w[hidden * d:hidden * d + hidden] + w[:hidden * d].reshape(hidden, d) @ x
        y = w[-a:] + w[hidden * d + hidden:-a].reshape(a, hidden) @ np.where(z > 0, z, 0.0)
    return sr.softmax64(y, scale)[action]


def lane64(kind, hp, hc, wp, wc, x, x_next, actions, reward, done, ended, old_prob, gamma, lam, scale, bars):
    """(vs, pg): v_s = V(x_s) + sum_{t >= s} gamma^(t-s) (prod_{s <= i < t} c_i) rho_t (r_t + gamma V(x_{t+1}) - V(x_t)) up to the episode's end; rho_s (r_s + gamma v_{s+1} - V(x_s))"""
    k, gamma, lam = len(reward), float(F(gamma)), float(F(lam))
    ratio = np.array([prob64(kind, hp, wp, x[j], actions[j], float(F(scale))) / float(old_prob[j]) for j in range(k)])
    v = np.array([forward64(kind, hc, wc, x[j]) for j in range(k)])
    v_next = np.array([0.0 if done[j] else forward64(kind, hc, wc, x_next[j]) for j in range(k)])
    delta = np.minimum(ratio, bars[0]) * (reward + gamma * v_next - v)
    c = lam * np.minimum(ratio, bars[1])
    vs = np.zeros(k)
    for s in range(k):
        weight = 1.0
        for t in range(s, k):
            vs[s] += weight * delta[t]
            if ended[t]:
                break
            weight *= gamma * c[t]
        vs[s] += v[s]
    vs_next = np.array([v_next[s] if ended[s] or s == k - 1 else vs[s + 1] for s in range(k)])
    return vs, np.minimum(ratio, bars[2]) * (reward + gamma * vs_next - v)
