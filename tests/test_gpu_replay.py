"""gymrs_replay_push / _sample / _update against tests/replay_ref.py, bit for bit: the draw over stores of one tile, of two with a
ragged end and of four, with priority patterns a tiled prefix sum can get wrong (entries beyond count hold the largest priority and must
weigh nothing); the push of rollout records across the ring's wrap and at unaligned heads; the update with duplicates and a skipped
index; and one chain transitions -> push -> sample -> q_gradient -> update against gymrs_q_lane on the reference's rows."""
import numpy as np
import pytest
import replay_ref as ref
import torch
from test_gpu_advantages import stride_of, upload
from test_gpu_closed_loop_table import DEV

pytestmark = pytest.mark.gpu
A, S, T = 1, 2, 4
NAN, BYTE = 0x7FC00ABC, 9  # the canaries of f32 rows (a bit pattern) and u8 rows
DIMS = {0: 4, 1: 2}
ROWS = ("s", "s_next", "action", "reward", "done", "priority")


def host_store(d, capacity, seed):
    rng = np.random.default_rng([seed, capacity])
    return dict(s=rng.standard_normal((d, capacity)).astype(np.float32), s_next=rng.standard_normal((d, capacity)).astype(np.float32),
                action=rng.integers(0, 2, capacity).astype(np.uint8), reward=rng.standard_normal(capacity).astype(np.float32),
                done=rng.integers(0, 2, capacity).astype(np.uint8), priority=rng.integers(0, ref.MAX_P + 1, capacity).astype(np.uint32))


def device_store(gymrs, host):
    dev = {k: upload(v) for k, v in host.items()}
    return dev, gymrs.Replay(*(dev[k].data_ptr() for k in ROWS), host["priority"].size)


def batch_rows(d, stride):
    f32 = lambda *shape: torch.full(shape, NAN, dtype=torch.int32, device=DEV)  # noqa: E731
    u8 = lambda *shape: torch.full(shape, BYTE, dtype=torch.uint8, device=DEV)  # noqa: E731
    rows = dict(obs=f32(d, stride), start_obs=f32(d, stride), reward=f32(stride), idx=f32(stride), prio=f32(stride), actions=u8(stride), done=u8(stride),
                total=torch.full((1,), -1, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    return rows


def sample_args(rows, stride):
    p = {k: v.data_ptr() for k, v in rows.items()}
    return dict(batch=dict(obs=p["obs"], actions=p["actions"], reward=p["reward"], done=p["done"], lane_stride=stride), start_obs=p["start_obs"],
                idx=p["idx"], prio=p["prio"], total=p["total"])


def check_batch(rows, host, idx, total, b):
    """every output row of a draw against the gather of `host` at idx; the padding lanes (all lanes, without mass) keep their canary"""
    got = {k: v.cpu().numpy() for k, v in rows.items()}
    assert int(got["total"][0]) == total and np.array_equal(got["idx"][:b].view(np.uint32), idx)
    keep = b if total else 0
    for k, canary in (("obs", NAN), ("start_obs", NAN), ("reward", NAN), ("actions", BYTE), ("done", BYTE), ("idx", NAN), ("prio", NAN)):
        assert (got[k][..., (b if k in ("idx", "prio") else keep):] == canary).all(), ("canary", k)
    if not total:
        assert (idx == ref.NONE).all() and not got["prio"][:b].any()
        return
    want = dict(obs=host["s_next"][:, idx], start_obs=host["s"][:, idx], reward=host["reward"][idx], actions=host["action"][idx], done=host["done"][idx],
                prio=host["priority"][idx])
    for k, w in want.items():
        assert np.array_equal(got[k][..., :b].view(w.dtype), w), k


STORES = [(16, 5), (4096, 4096), (4112, 4100), (3 * 4096 + 16, 3 * 4096 + 1)]


@pytest.mark.parametrize("capacity,count,pattern", [(cap, count, name) for cap, count in STORES for name in ref.patterns(count)])
def test_draw(gymrs, capacity, count, pattern):
    prio = ref.patterns(count)[pattern]
    kind = 1 if capacity == 4112 else 0
    host = host_store(DIMS[kind], capacity, 3)
    host["priority"][:count], host["priority"][count:] = prio, ref.MAX_P
    dev, store = device_store(gymrs, host)
    store.count = count
    eng = gymrs.BatchedEngine(kind, 16, flags=A)
    for b in (1, 7, count, 3 * count):
        stride = stride_of(b)
        rows = batch_rows(DIMS[kind], stride)
        eng.replay_sample(store, b, seed=0xC0FFEE, draw=b, **sample_args(rows, stride))
        eng.sync()
        idx, total = ref.draw(prio, b, 0xC0FFEE, b)
        check_batch(rows, host, idx, total, b)
    for k, v in dev.items():
        assert np.array_equal(v.cpu().numpy().view(host[k].dtype), host[k]), ("the store was written", k)
    eng.close()


_records = {}


def collected(gymrs, kind):
    """36 exploring steps of 4200 lanes under a short time limit, on the host: obs [K][D][n], start_obs [D][n], ..."""
    if kind not in _records:
        n, steps, d, s = 4200, 36, DIMS[kind], stride_of(4200)
        p = gymrs.engine.default_params(kind)
        p.max_episode_steps = 16 if kind == 0 else 5
        eng = gymrs.BatchedEngine(kind, n, params=p, flags=A | S | T)
        eng.reset(seed=3)
        eng.set_policy(np.zeros((1, gymrs.policy_size(kind, 0)), np.float32), lanes_per_policy=n)
        eng.set_exploration(5, epsilon=1.0)
        f32 = lambda *shape: torch.full(shape, NAN, dtype=torch.int32, device=DEV)  # noqa: E731
        u8 = lambda *shape: torch.full(shape, BYTE, dtype=torch.uint8, device=DEV)  # noqa: E731
        t = dict(obs=f32(steps, d, s), final_obs=f32(steps, d, s), start_obs=f32(d, s), reward=f32(steps, s), actions=u8(steps, s), done=u8(steps, s),
                 truncated=u8(steps, s))
        torch.cuda.synchronize()
        record = {k: t[k].data_ptr() for k in ("obs", "actions", "reward", "done", "truncated")}
        eng.rollout_transitions(steps, record=dict(record, lane_stride=s), final_obs=t["final_obs"].data_ptr(), start_obs=t["start_obs"].data_ptr(), explore=True)
        eng.sync()
        eng.close()
        _records[kind] = {k: v.cpu().numpy()[..., :n] for k, v in t.items()}
        _records[kind].update({k: v.view(np.uint32) for k, v in _records[kind].items() if v.dtype == np.int32})  # f32 rows stay bit patterns
    return _records[kind]


def cut(c, lanes, k0, steps):
    """steps [k0, k0 + steps) of the chosen lanes as a record of its own"""
    out = {k: c[k][k0:k0 + steps][..., lanes] for k in ("obs", "final_obs", "reward", "actions", "done", "truncated")}
    out["start_obs"] = c["obs"][k0 - 1][..., lanes]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}  # (an index array leaves the lanes outermost in memory)


@pytest.mark.parametrize("head", [0, 3, -1])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("n", [5, 4200])
@pytest.mark.parametrize("kind", [0, 1])
def test_push(gymrs, kind, n, steps, head):
    c, d = collected(gymrs, kind), DIMS[kind]
    done, trunc = c["done"] != 0, (c["truncated"] != 0) & (c["done"] == 0)
    # a step at which lanes are done, truncated and going on (MountainCar never finishes here and truncates all lanes at once)
    k0 = next(k for k in range(20, 33) if trunc[k].any() and (kind == 1 or (done[k].any() and not (done[k] | trunc[k]).all())))
    lanes = np.arange(n)
    if n == 5 and kind == 0:  # a done, a truncated and three going-on lanes, the ended ones in the middle
        on = np.flatnonzero(~done[k0] & ~trunc[k0])
        lanes = np.concatenate([on[:2], np.flatnonzero(done[k0])[:1], np.flatnonzero(trunc[k0])[:1], on[2:3]])
    r = cut(c, lanes, k0, steps)
    if kind == 0:
        ended = (r["done"] != 0) | (r["truncated"] != 0)
        assert (r["done"] != 0).any() and ((r["truncated"] != 0) & (r["done"] == 0)).any() and not ended.all()
    capacity = (steps * n + 15) // 16 * 16 + 32
    head = head if head >= 0 else capacity - n - 1  # the last one crosses the wrap
    f32, u8 = (lambda *shape: np.full(shape, NAN, np.uint32)), (lambda *shape: np.full(shape, BYTE, np.uint8))
    host = dict(s=f32(d, capacity), s_next=f32(d, capacity), action=u8(capacity), reward=f32(capacity), done=u8(capacity), priority=f32(capacity))
    dev, store = device_store(gymrs, host)
    stride = stride_of(n)
    rows = {k: upload(np.pad(v, [(0, 0)] * (v.ndim - 1) + [(0, stride - n)], constant_values=BYTE)) for k, v in r.items()}
    eng = gymrs.BatchedEngine(kind, n, flags=A)
    store.head = head
    eng.replay_push(store, steps, record=dict({k: rows[k].data_ptr() for k in ("obs", "actions", "reward", "done", "truncated")}, lane_stride=stride),
                    start_obs=rows["start_obs"].data_ptr(), final_obs=rows["final_obs"].data_ptr(), priority=12345)
    eng.sync()
    assert (store.head, store.count) == ((head + steps * n) % capacity, steps * n)
    want = ref.flatten(dict(r, priority=12345), n, steps, head, capacity, host)
    for k in ROWS:
        got = dev[k].cpu().numpy().view(want[k].dtype)
        assert np.array_equal(got, want[k]), (k, np.argwhere(got != want[k])[:4])
    eng.close()


def test_update(gymrs):
    capacity, b = 4112, 300
    rng = np.random.default_rng(11)
    host = host_store(4, capacity, 2)
    dev, store = device_store(gymrs, host)
    idx = rng.integers(0, capacity, b).astype(np.uint32)
    idx[10:20] = idx[0:10]  # duplicates carry the same td
    per_entry = (rng.standard_normal(capacity) * 3).astype(np.float32)
    per_entry[idx[:4]] = [np.nan, np.inf, -np.inf, 0.0]
    td = per_entry[idx]
    idx[50] = ref.NONE
    eng = gymrs.BatchedEngine(0, 16, flags=A)
    rows = upload(idx), upload(td)
    eng.replay_update(store, b, idx=rows[0].data_ptr(), td=rows[1].data_ptr(), alpha=0.6, eps=1e-3, cap=4.0)
    eng.sync()
    want, keep = host["priority"].copy(), np.delete(np.arange(b), 50)
    want[idx[keep]] = ref.priority(td[keep], 0.6, 1e-3, 4.0)
    assert np.array_equal(dev["priority"].cpu().numpy().view(np.uint32), want) and len(set(want[idx[keep]])) > 100
    eng.close()


def test_chain(gymrs):
    """transitions, push, sample, q_gradient with final_obs = batch.obs, update: td and the table are gymrs_q_lane's on the reference's
    sampled rows, the new priorities are the rule's on that td, and the next draw follows them"""
    kind, d, n, steps, capacity, hidden = 0, 4, 256, 4, 4112, 5
    size, stride = gymrs.policy_size(kind, hidden), stride_of(n)
    rng = np.random.default_rng(5)
    target, online = (rng.standard_normal((1, size)).astype(np.float32) * np.float32(0.5) for _ in range(2))
    eng = gymrs.BatchedEngine(kind, n, flags=A | S | T)
    eng.reset(seed=9)
    eng.set_policy(target, hidden=hidden, lanes_per_policy=n)
    eng.q_target_sync()
    eng.set_policy(online, hidden=hidden, lanes_per_policy=n)
    eng.set_exploration(3, epsilon=0.5)
    c = {k: torch.zeros(shape, dtype=dt, device=DEV) for k, shape, dt in (("obs", (steps, d, stride), torch.float32), ("final_obs", (steps, d, stride), torch.float32),
         ("start_obs", (d, stride), torch.float32), ("reward", (steps, stride), torch.float32), ("actions", (steps, stride), torch.uint8),
         ("done", (steps, stride), torch.uint8), ("truncated", (steps, stride), torch.uint8))}
    host = {k: np.zeros_like(v) for k, v in host_store(d, capacity, 1).items()}
    dev, store = device_store(gymrs, host)
    rows, td = batch_rows(d, stride), torch.zeros(stride, dtype=torch.float32, device=DEV)
    tables = dict(grad=torch.zeros((1, size), dtype=torch.int64, device=DEV), excluded=torch.zeros(1, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    record = dict({k: c[k].data_ptr() for k in ("obs", "actions", "reward", "done", "truncated")}, lane_stride=stride)
    eng.rollout_transitions(steps, record=record, final_obs=c["final_obs"].data_ptr(), start_obs=c["start_obs"].data_ptr(), explore=True)
    eng.replay_push(store, steps, record=record, start_obs=c["start_obs"].data_ptr(), final_obs=c["final_obs"].data_ptr())
    args = sample_args(rows, stride)
    eng.replay_sample(store, n, seed=77, draw=0, **args)
    eng.q_gradient(1, record=dict(args["batch"]), start_obs=args["start_obs"], final_obs=args["batch"]["obs"], td=td.data_ptr(), gamma=0.97, kappa=1.0,
                   **{k: v.data_ptr() for k, v in tables.items()})
    eng.replay_update(store, n, idx=args["idx"], td=td.data_ptr(), alpha=0.6, eps=1e-3, cap=2.0)
    eng.sync()
    r = {k: v.cpu().numpy()[..., :n] for k, v in c.items()}
    st = ref.flatten(dict(r, priority=ref.MAX_P), n, steps, 0, capacity, host)
    idx, total = ref.draw(st["priority"][:steps * n], n, 77, 0)
    check_batch(rows, st, idx, total, n)
    lanes = [gymrs.q_lane(kind, hidden, online[0], target[0], st["s"][:, e][None], st["s_next"][:, e][None], st["action"][[e]], st["reward"][[e]],
                          st["done"][[e]], gamma=0.97, kappa=1.0) for e in idx]
    want_td = np.array([o[2][0] for o in lanes], np.float32)
    assert np.array_equal(td.cpu().numpy()[:n].view(np.uint32), want_td.view(np.uint32)) and want_td.any()
    assert np.array_equal(tables["grad"].cpu().numpy()[0], np.sum([o[0] for o in lanes], axis=0)) and not tables["excluded"].cpu().numpy().any()
    st["priority"][idx] = ref.priority(want_td, 0.6, 1e-3, 2.0)
    assert np.array_equal(dev["priority"].cpu().numpy().view(np.uint32), st["priority"])
    again = batch_rows(d, stride)
    eng.replay_sample(store, n, seed=77, draw=1, **sample_args(again, stride))
    eng.sync()
    check_batch(again, st, *ref.draw(st["priority"][:steps * n], n, 77, 1), n)
    eng.close()
