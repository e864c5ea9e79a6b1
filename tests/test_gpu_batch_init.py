"""Lane initialisation (hpe_pso_optimise_batch, hpe_batch_pipeline_optimise): pso_optimise of
every lane of a batch in the same launches.

The yardstick is always hpe_pso_optimise on a SEPARATE context created with that lane's hand,
under the same seed and PSO parameters, on the same frame; every comparison is np.array_equal on
bestp, the cost and the whole gbest trace.  Frames are rendered with oracle_np.render_depth_mm
from hand_data.trajectory and preprocessed once on the host (downsampled, 250 points, unless
stated); every context stores the same arrays.  A yardstick is computed once and shared.

Small shapes: at most a few dozen launches of at most 512 workgroups per case.
"""
import ctypes as C

import numpy as np
import pytest

import hand_data

pytestmark = pytest.mark.gpu

FOCAL, MXY, MZ = 241.42, 1.0, 2.0
SENTINEL = -7.0
SCALES = {"S": (0.9, 0.85), "L": (1.1, 1.2), "M": (1.05, 0.95)}


def _np_hand(name):
    import oracle_np
    geo, rad = hand_data.geometry_cm()
    if name == "A":
        return oracle_np.Hand(geo, rad)
    s, rs = SCALES[name]
    return oracle_np.Hand(geo * s, rad * rs)


class Frames:
    """The frames of the file: raw (float32 mm) and preprocessed on the host, by key."""

    def __init__(self):
        import hpe
        import oracle_np
        self.hpe = hpe
        self.raw, self.obs = {}, {}
        poses = hand_data.trajectory(6, seed=3)
        self.pose = {}
        for k in range(4):  # a0 .. a3: the reference hand
            self._render("a%d" % k, "A", poses[k + 1])
        for name, seed in (("S", 5), ("L", 6), ("M", 7)):  # s0, s1 / l0, l1 / m0: a hand of that size
            p = hand_data.trajectory(3, seed=seed)
            for k in range(1 if name == "M" else 2):
                self._render("%s%d" % (name.lower(), k), name, p[k + 1])
        # other cloud sizes, from a0's full-resolution cloud: 400 points (LDS above the 250-point
        # lanes'), 100 points (a cropped hand), and the full cloud (above 2048: refused)
        full = hpe.preprocess_depth(self.raw["a0"], True, False, FOCAL)
        n = len(full["cloud"])
        assert n > 2048
        for key, m in (("n400", 400), ("n100", 100)):
            d = dict(full)
            d["cloud"] = full["cloud"][np.linspace(0, n - 1, m).astype(int)].copy()
            self.obs[key] = d
        self.obs["full"] = full
        self.X0 = np.asarray(oracle_np.X0, dtype=np.float64)

    def _render(self, key, hand, pose):
        import oracle_np
        d = np.ascontiguousarray(oracle_np.render_depth_mm(_np_hand(hand), pose), dtype=np.float32)
        self.raw[key] = d
        self.pose[key] = pose
        self.obs[key] = self.hpe.preprocess_depth(d, True, True, FOCAL)

    def x0(self, k):
        """Start k: the reference start, moved a little (k = 0: as it is)."""
        x = self.X0.copy()
        x[:3] += 0.4 * k * np.array([1.0, -0.5, 0.25])
        x[6:] += 0.5 * k
        return x


class Env:
    """One context created with hand `name`: the single call (the yardstick) or the lane calls."""

    def __init__(self, name, frames, params=True):
        import hpe
        import torch
        from hpe import _lib, window
        self.hpe, self.torch, self._lib, self.window = hpe, torch, _lib, window
        self.name, self.frames = name, frames
        self.hand = hpe.reference_hand(device=0) if name == "A" else hpe.scaled_hand(*SCALES[name])
        self.ctx = self.hand.ctx
        self.lib, self.h = self.ctx.lib, self.ctx.h
        self.slots = {}
        self.maxiter = None
        if params:
            self.params(3)

    def params(self, maxiter):
        if maxiter != self.maxiter:
            ub, lb, sd = self.hpe.reference_bounds()
            pso = self.hpe.PSO()
            pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, maxiter, 1e-8, 1e-8)
            pso._push(self.ctx)
            self.maxiter = maxiter

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.h))

    def slot(self, key):
        """The host-preprocessed frame `key` stored in a slot of this context, once."""
        if key not in self.slots:
            d = self.frames.obs[key]
            s = 8 + len(self.slots)
            self.ctx.store_frame(s, d["depth_cm"], d["dt"], d["cloud"], d["scale"], d["dtmax"], d["K"])
            self.slots[key] = s
        return self.slots[key]

    def dev_slot(self, depth_mm):
        """A raw frame prepared on the device into a fresh slot."""
        s = 8 + len(self.slots)
        self.slots[("dev", s)] = s
        self.ctx.prepare_frame(s, depth_mm)
        return s

    def single_on_slot(self, slot, x0, P, maxiter):
        """hpe_pso_optimise on a slot: ({bestp, cost} as 27 doubles, the trace)."""
        self.params(maxiter)
        self.ctx.select_frame(slot)
        G = max(maxiter - 1, 0)
        x = np.ascontiguousarray(x0, dtype=np.float64)
        out, bc, tr = np.zeros(27), C.c_double(0), np.zeros(max(G, 1))
        self.ctx.check(self.lib.hpe_pso_optimise(self.h, self._lib.ptr(x, C.c_double), int(P),
                                                 self._lib.ptr(out, C.c_double), C.byref(bc),
                                                 self._lib.ptr(tr, C.c_double), G))
        out[26] = bc.value
        return out, tr[:G].copy()

    def rows(self, x0s):
        r = np.full((len(x0s), 27), SENTINEL)
        r[:, :26] = np.asarray(x0s)
        return r

    def device(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def trace_buf(self, B, maxiter):
        return self.torch.full((B, max(maxiter - 1, 1)), SENTINEL, dtype=self.torch.float64,
                               device="cuda:0")

    def batch(self, P, maxiter, keys, x0s):
        """hpe_pso_optimise_batch over the frames `keys`: (states B x 27, traces B x G)."""
        self.params(maxiter)
        st, tr = self.device(self.rows(x0s)), self.trace_buf(len(keys), maxiter)
        self.torch.cuda.synchronize()
        self.ctx.pso_optimise_batch(P, st.data_ptr(), [self.slot(k) for k in keys], tr.data_ptr())
        self.sync()
        return st.cpu().numpy(), tr.cpu().numpy()[:, :max(maxiter - 1, 0)]


class Pool:
    def __init__(self):
        self.frames = Frames()
        self.envs = {}
        self.yards = {}
        self.batch_env = Env("A", self.frames)  # the context under test, never a yardstick

    def env(self, name):
        if name not in self.envs:
            self.envs[name] = Env(name, self.frames)
        return self.envs[name]

    def yard(self, hand, key, k, P, maxiter):
        """The single call of hand `hand`'s own context on frame `key` from start k."""
        q = (hand, key, k, P, maxiter)
        if q not in self.yards:
            e = self.env(hand)
            self.yards[q] = e.single_on_slot(e.slot(key), self.frames.x0(k), P, maxiter)
        return self.yards[q]

    def set_hands(self, env, names):
        env.ctx.set_batch_hands(None if names is None else [self.env(h).hand for h in names])

    def close(self):
        self.batch_env.ctx.close()
        for e in self.envs.values():
            e.ctx.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


@pytest.fixture()
def env(pool):
    e = pool.batch_env
    yield e
    try:
        e.ctx.set_batch_hands(None)
    except e.hpe.HpeError:
        pass  # a live batch a failed test left behind keeps its hands


def check_lane(got, b, want, what):
    st, tr = got
    assert np.array_equal(st[b, :26], want[0][:26]), ("bestp", what)
    assert st[b, 26] == want[0][26], ("cost", what)
    assert np.array_equal(tr[b], want[1]), ("trace", what)


# ---- 1. three lanes on stored slots
@pytest.mark.parametrize("P,maxiter", [(16, 4), (5, 3), (17, 3), (1, 2), (16, 1)])
def test_three_lanes_on_slots(pool, env, P, maxiter):
    """P = ARRIVE_SHARDS, below it, not a multiple of it, one particle; one generation
    (maxiter 2) and none (maxiter 1: the initial swarm's best, as in the single call)."""
    keys, ks = ["a0", "a1", "a2"], [0, 1, 2]
    got = env.batch(P, maxiter, keys, [pool.frames.x0(k) for k in ks])
    yards = [pool.yard("A", key, k, P, maxiter) for key, k in zip(keys, ks)]
    for b in range(3):
        check_lane(got, b, yards[b], (P, maxiter, b))
    assert np.isfinite(got[0]).all() and got[1].shape == (3, maxiter - 1)
    assert not np.array_equal(yards[0][0], yards[1][0])
    assert not np.array_equal(yards[1][0], yards[2][0])


# ---- 2. sixteen lanes: test_full's particle count, 512 workgroups
@pytest.mark.parametrize("odd", [15, 0])
def test_sixteen_lanes_one_odd_frame(pool, env, odd):
    keys = ["a0"] * 16
    keys[odd] = "a1"
    got = env.batch(32, 3, keys, [pool.frames.x0(0)] * 16)
    ya, yo = pool.yard("A", "a0", 0, 32, 3), pool.yard("A", "a1", 0, 32, 3)
    for b in range(16):
        check_lane(got, b, yo if b == odd else ya, (odd, b))
    assert not np.array_equal(ya[0], yo[0])


def test_sixteen_lanes_permuted(pool, env):
    lanes = [("a%d" % (b % 4), b % 3) for b in range(16)]
    perm = [5, 12, 0, 9, 3, 15, 7, 1, 14, 10, 2, 8, 13, 4, 11, 6]
    run = lambda ls: env.batch(32, 3, [k for k, _ in ls], [pool.frames.x0(s) for _, s in ls])
    first = run(lanes)
    second = run([lanes[p] for p in perm])
    for b, (key, k) in enumerate(lanes):
        check_lane(first, b, pool.yard("A", key, k, 32, 3), b)
    for b, p in enumerate(perm):
        assert np.array_equal(second[0][b], first[0][p]) and np.array_equal(second[1][b], first[1][p])


# ---- 3. clouds of different sizes in one launch
def test_mixed_cloud_sizes(pool, env):
    """The 400-point lane sizes the descent's dynamic LDS; the 100- and 250-point lanes size
    their arrays by their own n and equal their single calls."""
    keys = ["n100", "n400", "a0"]
    assert [len(pool.frames.obs[k]["cloud"]) for k in keys] == [100, 400, 250]
    for order in ([0, 1, 2], [1, 2, 0]):
        ks = [keys[i] for i in order]
        got = env.batch(16, 3, ks, [pool.frames.x0(0)] * 3)
        for b, key in enumerate(ks):
            check_lane(got, b, pool.yard("A", key, 0, 16, 3), (order, key))
    assert not np.array_equal(pool.yard("A", "n100", 0, 16, 3)[0], pool.yard("A", "a0", 0, 16, 3)[0])


# ---- 4. lane hands
def test_lane_hands_on_slots(pool, env):
    names, keys = ["M", "S", "L"], ["m0", "s0", "l0"]  # three hands from hpe.scaled_hand
    x0s = [pool.frames.x0(0)] * 3
    own_before = env.single_on_slot(env.slot("a3"), pool.frames.x0(1), 16, 3)
    pool.set_hands(env, names)
    got = env.batch(16, 3, keys, x0s)
    for b, h in enumerate(names):
        check_lane(got, b, pool.yard(h, keys[b], 0, 16, 3), h)
    # the hand matters: on one frame the three hands' results differ
    same = [pool.yard(h, "s0", 0, 16, 3)[0] for h in names]
    assert not np.array_equal(same[0], same[1]) and not np.array_equal(same[1], same[2])
    # the context's own single call does not see the table, and keeps its selected frame
    own_during = env.single_on_slot(env.slot("a3"), pool.frames.x0(1), 16, 3)
    # hands = NULL: every lane under the context's hand
    pool.set_hands(env, None)
    got = env.batch(16, 3, keys, x0s)
    for b in range(3):
        check_lane(got, b, pool.yard("A", keys[b], 0, 16, 3), ("no hands", b))
    own_after = env.single_on_slot(env.slot("a3"), pool.frames.x0(1), 16, 3)
    for o in (own_during, own_after):
        assert np.array_equal(o[0], own_before[0]) and np.array_equal(o[1], own_before[1])
    want = pool.yard("A", "a3", 1, 16, 3)
    assert np.array_equal(own_before[0], want[0]) and np.array_equal(own_before[1], want[1])


def test_the_selected_frame_stays(pool, env):
    """The slot call selects nothing: hpe_pso_optimise right after it runs on the frame selected
    before it."""
    env.params(3)
    env.ctx.select_frame(env.slot("a3"))
    env.batch(16, 3, ["a0", "a1"], [pool.frames.x0(0)] * 2)
    x = pool.frames.x0(1)
    out, bc, tr = np.zeros(27), C.c_double(0), np.zeros(2)
    ptr = env._lib.ptr
    env.ctx.check(env.lib.hpe_pso_optimise(env.h, ptr(x, C.c_double), 16, ptr(out, C.c_double),
                                           C.byref(bc), ptr(tr, C.c_double), 2))
    want = pool.yard("A", "a3", 1, 16, 3)
    assert np.array_equal(out[:26], want[0][:26]) and bc.value == want[0][26]
    assert np.array_equal(tr, want[1])


# ---- 5. the counters are left ready; the arenas grow and are rebuilt
def test_twice_in_a_row_and_after_a_different_shape(pool, env):
    keys, x0s = ["a0", "a1", "a2"], [pool.frames.x0(k) for k in range(3)]
    first = env.batch(16, 3, keys, x0s)
    second = env.batch(16, 3, keys, x0s)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    small = env.batch(5, 3, keys[:2], x0s[:2])
    for b in range(2):
        check_lane(small, b, pool.yard("A", keys[b], b, 5, 3), ("P 5", b))
    grown = env.batch(16, 4, keys + ["a3"], x0s + [pool.frames.x0(0)])  # more lanes, longer trace
    for b in range(3):
        check_lane(grown, b, pool.yard("A", keys[b], b, 16, 4), ("grown", b))
    check_lane(grown, 3, pool.yard("A", "a3", 0, 16, 4), ("grown", 3))
    third = env.batch(16, 3, keys, x0s)
    assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1])


# ---- 6. a live batch: windows and hands, and nothing of the batch disturbed
def test_live_batch_with_fixed_windows_and_hands(pool, env):
    P, maxiter = 16, 3
    names = ["A", "S", "L"]
    fr = [[pool.frames.raw["%s%d" % (h.lower(), k)] for k in range(2)] for h in names]
    x0 = pool.frames.x0(0)
    wins, masked = [], []
    for b, h in enumerate(names):
        e = pool.env(h)
        w = e.ctx.window_from_pose(pool.frames.pose["%s0" % h.lower()], FOCAL, MXY, MZ)
        w = w._replace(row_hi=w.row_hi - 15)  # crops the wrist end: the mask changes the frame
        wins.append(w)
        masked.append([e.window.apply(f, w) for f in fr[b]])
        assert not np.array_equal(masked[b][0], fr[b][0])
    # the yardsticks: the single call on the host-masked frame, then the single pipelined loop
    yards = []
    for b, h in enumerate(names):
        e = pool.env(h)
        opt = e.single_on_slot(e.dev_slot(masked[b][0]), x0, P, maxiter)
        st1 = e.device(opt[0])
        e.ctx.pipeline_begin(masked[b][0])
        states = []
        for f in range(2):
            e.ctx.track_pipelined(P, 1, st1.data_ptr(), masked[b][1] if f == 0 else None)
            e.sync()
            states.append(st1.cpu().numpy().copy())
        yards.append((opt, states))
    env.params(maxiter)
    pool.set_hands(env, names)
    env.ctx.set_batch_window("fixed", wins)
    try:
        st, tr = env.device(env.rows([x0] * 3)), env.trace_buf(3, maxiter)
        env.ctx.batch_pipeline_begin([f[0] for f in fr])
        env.ctx.batch_pipeline_optimise(P, st.data_ptr(), None, tr.data_ptr())
        env.sync()
        got = (st.cpu().numpy(), tr.cpu().numpy())
        for b, h in enumerate(names):
            check_lane(got, b, yards[b][0], ("live", h))
        for f in range(2):
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [x[1] for x in fr] if f == 0 else None)
            env.sync()
            now = st.cpu().numpy()
            for b, h in enumerate(names):
                assert np.array_equal(now[b], yards[b][1][f]), (h, f)
    finally:
        try:
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)  # ends a batch left alive
        except env.hpe.HpeError:
            pass
        env.sync()
        env.ctx.set_batch_window("off")
    assert not np.array_equal(yards[0][0][0], yards[1][0][0])


# ---- 7. a subset of the lanes; a lane that joins late
def test_subset_and_pacing(pool, env):
    P, maxiter = 16, 3
    _lib = env._lib
    raw, x0 = pool.frames.raw, pool.frames.x0(0)
    ya = pool.env("A")
    yard = lambda key: ya.single_on_slot(ya.dev_slot(raw[key]), x0, P, maxiter)
    y0, y2, y1 = yard("a0"), yard("a2"), yard("a1")
    env.params(maxiter)
    pattern = np.arange(27, dtype=np.float64) * -3.5 - 1234.0625
    rows = env.rows([x0] * 3)
    rows[1] = pattern
    st, tr = env.device(rows), env.trace_buf(3, maxiter)
    env.ctx.set_batch_pacing("free")
    try:
        env.ctx.batch_pipeline_begin([raw["a0"], None, raw["a2"]])
        assert env.ctx.batch_pending() == 0b101
        # lane 1 holds no frame: selecting it is refused and changes nothing
        for lanes in (0b010, 0b111):
            rc = env.lib.hpe_batch_pipeline_optimise(env.h, P, 3, C.c_void_p(st.data_ptr()), lanes,
                                                     C.c_void_p(tr.data_ptr()))
            assert rc == _lib.HPE_E_STATE and b"no prepared frame" in env.lib.hpe_last_error(env.h)
        env.sync()
        assert np.array_equal(st.cpu().numpy(), rows)
        assert (tr.cpu().numpy() == SENTINEL).all()
        env.ctx.batch_pipeline_optimise(P, st.data_ptr(), 0b101, tr.data_ptr())
        env.sync()
        got = (st.cpu().numpy(), tr.cpu().numpy())
        check_lane(got, 0, y0, "lane 0")
        check_lane(got, 2, y2, "lane 2")
        assert np.array_equal(got[0][1], pattern) and (got[1][1] == SENTINEL).all()
        # lanes=None under free pacing: the pending lanes, the same result
        st2, tr2 = env.device(rows), env.trace_buf(3, maxiter)
        env.ctx.batch_pipeline_optimise(P, st2.data_ptr(), None, tr2.data_ptr())
        env.sync()
        assert np.array_equal(st2.cpu().numpy(), got[0]) and np.array_equal(tr2.cpu().numpy(), got[1])
        assert env.ctx.batch_pending() == 0b101  # nothing of the batch moved
        # lane 1 joins: its frame arrives in a track call, into the other buffer parity
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [raw["a3"], raw["a1"], raw["a3"]])
        env.sync()
        assert env.ctx.batch_pending() == 0b111
        mid = st.cpu().numpy()
        assert np.array_equal(mid[1], pattern)
        assert not np.array_equal(mid[0], got[0][0])  # lanes 0 and 2 tracked a frame
        st[1] = env.device(env.rows([x0]))[0]
        tr.fill_(SENTINEL)
        env.torch.cuda.synchronize()
        env.ctx.batch_pipeline_optimise(P, st.data_ptr(), 0b010, tr.data_ptr())
        env.sync()
        got = (st.cpu().numpy(), tr.cpu().numpy())
        check_lane(got, 1, y1, "lane 1 joined")
        assert np.array_equal(got[0][0], mid[0]) and np.array_equal(got[0][2], mid[2])
        assert (got[1][0] == SENTINEL).all() and (got[1][2] == SENTINEL).all()
    finally:
        try:
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)
        except env.hpe.HpeError:
            pass
        env.sync()
        env.ctx.set_batch_pacing("lockstep")


# ---- 8. refusals change nothing
def test_refusals_change_nothing(pool, env):
    _lib, lib, h = env._lib, env.lib, env.h
    M = _lib.BATCH_MAX
    P, maxiter = 16, 3
    keys, x0s = ["a0", "a1", "a2"], [pool.frames.x0(k) for k in range(3)]
    want = env.batch(P, maxiter, keys, x0s)
    for b in range(3):
        check_lane(want, b, pool.yard("A", keys[b], b, P, maxiter), b)

    def err():
        return lib.hpe_last_error(h)

    def still():
        got = env.batch(P, maxiter, keys, x0s)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

    rows = env.rows(x0s)
    st = env.device(np.vstack([rows] * 6)[:M + 1])
    sp = C.c_void_p(st.data_ptr())
    good = (C.c_int32 * (M + 1))(*[env.slot("a0")] * (M + 1))

    def slots(*s):
        return (C.c_int32 * len(s))(*s)

    def untouched():
        env.sync()
        assert np.array_equal(st.cpu().numpy()[:3], rows)

    # the slot call
    for B in (0, M + 1, -1):
        assert lib.hpe_pso_optimise_batch(h, P, B, sp, good, None) == _lib.HPE_E_ARG and b"lanes" in err()
    assert lib.hpe_pso_optimise_batch(h, P, 3, None, good, None) == _lib.HPE_E_ARG
    assert lib.hpe_pso_optimise_batch(h, P, 3, sp, None, None) == _lib.HPE_E_ARG
    for bad in (4000, -1, 5000):
        assert lib.hpe_pso_optimise_batch(h, P, 3, sp, slots(env.slot("a0"), bad, env.slot("a1")),
                                          None) == _lib.HPE_E_ARG and b"holds no frame" in err()
    assert lib.hpe_pso_optimise_batch(h, P, 2, sp, slots(env.slot("a0"), env.slot("full")),
                                      None) == _lib.HPE_E_ARG and b"points" in err()
    for bad_p in (0, 8193):
        assert lib.hpe_pso_optimise_batch(h, bad_p, 3, sp, good, None) == _lib.HPE_E_ARG
        assert b"num_p" in err()
    untouched()
    still()
    pool.set_hands(env, ["A", "S"])
    assert lib.hpe_pso_optimise_batch(h, P, 3, sp, good, None) == _lib.HPE_E_STATE
    assert b"hands were set for 2" in err()
    pool.set_hands(env, None)
    untouched()
    still()
    # the live call: no live batch, then a lockstep batch of 3 lanes
    assert lib.hpe_batch_pipeline_optimise(h, P, 3, sp, 0b111, None) == _lib.HPE_E_STATE
    assert b"no live batch" in err()
    raw = pool.frames.raw
    env.ctx.batch_pipeline_begin([raw["a0"], raw["a1"], raw["a2"]])
    try:
        for B, lanes, code in ((0, 1, _lib.HPE_E_ARG), (M + 1, 1, _lib.HPE_E_ARG),
                               (3, 0, _lib.HPE_E_ARG), (3, 0b1000, _lib.HPE_E_ARG),
                               (3, 1 << 31, _lib.HPE_E_ARG), (2, 0b11, _lib.HPE_E_STATE),
                               (4, 0b1111, _lib.HPE_E_STATE)):
            assert lib.hpe_batch_pipeline_optimise(h, P, B, sp, lanes, None) == code, (B, lanes)
        assert lib.hpe_batch_pipeline_optimise(h, P, 3, None, 0b111, None) == _lib.HPE_E_ARG
        assert lib.hpe_batch_pipeline_optimise(h, 0, 3, sp, 0b111, None) == _lib.HPE_E_ARG
        untouched()
        # the batch is as it was: a good call, then its frames track
        ya = pool.env("A")
        y = [ya.single_on_slot(ya.dev_slot(raw[k]), x0s[b], P, maxiter) for b, k in enumerate(keys)]
        env.params(maxiter)
        tr = env.trace_buf(3, maxiter)
        env.ctx.batch_pipeline_optimise(P, st.data_ptr(), 0b111, tr.data_ptr())
        env.sync()
        got = (st.cpu().numpy(), tr.cpu().numpy())
        for b in range(3):
            check_lane(got, b, y[b], ("live after refusals", b))
    finally:
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)
        env.sync()
    still()
    # a context whose PSO parameters were never set
    bare = Env("A", pool.frames, params=False)
    try:
        s = bare.slot("a0")
        bst = bare.device(rows)
        bsp = C.c_void_p(bst.data_ptr())
        assert bare.lib.hpe_pso_optimise_batch(bare.h, P, 3, bsp, slots(s, s, s), None) == _lib.HPE_E_STATE
        assert b"hpe_set_pso_params" in bare.lib.hpe_last_error(bare.h)
        assert bare.lib.hpe_batch_pipeline_optimise(bare.h, P, 3, bsp, 0b111, None) == _lib.HPE_E_STATE
        bare.sync()
        assert np.array_equal(bst.cpu().numpy(), rows)
    finally:
        bare.ctx.close()


# ---- 9. the result never depends on the arrival order
def test_sixteen_lanes_three_times(pool, env):
    lanes = [("a%d" % (b % 4), b % 3) for b in range(16)]
    runs = [env.batch(32, 3, [k for k, _ in lanes], [pool.frames.x0(s) for _, s in lanes])
            for _ in range(3)]
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])
    assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][1]).all()
