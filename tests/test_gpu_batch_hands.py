"""Lane hands (hpe_set_batch_hands): every lane of the prepared, raw and live batch tracks with a
hand model of its own.

The yardstick is always the batch call's single-sequence counterpart on a SEPARATE context created
with that lane's hand (same seed, PSO parameters and refine form), compared with np.array_equal on
whole histories and final states; never the batch itself.  A lane's frames are rendered once, by
the default yardstick context of its hand, so the tracker sees a hand of its model's size.

Hands: A the reference hand, S = scaled_hand(0.9, 0.85), L = scaled_hand(1.1, 1.2), and V, which
also moves cmc_deg and spacing_cm: hand_data.hand_family()["V"].  Both oracles mirror V
(oracle.hand / oracle_np.Hand take cmc and spacing), and tests/test_gpu_hand_family.py compares
V's FK, costs, optimisers and lanes with them; this file keeps the bit-identity yardstick.  Hand h
tracks hpe.synth.trajectory seed SEED[h].

Small shapes: P = 32, maxiter 4 (G = 3), 250-point clouds, at most 5 frames per lane, chunks of 2
frames plus a tail.  Contexts are created when first needed and shared by the file.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF, K = 32, 4, 5, 2
FOCAL, MXY, MZ = 241.42, 1.0, 2.0
SENTINEL = -7.0
SEED = {"A": 0, "S": 1, "L": 2, "V": 1}
SCALES = {"S": (0.9, 0.85), "L": (1.1, 1.2)}


def make_hand(name):
    import hpe
    if name == "A":
        return hpe.reference_hand(device=0)
    if name in SCALES:
        return hpe.scaled_hand(*SCALES[name])
    assert name == "V"
    import hand_data
    return hand_data.family_gpu_hand(hand_data.hand_family()["V"])


class Env:
    """One context created with hand `name` (under HPE_PSO_FORM / HPE_PSO_WPP if given): the
    single-sequence calls -- the yardsticks -- and the batch calls."""

    def __init__(self, name, form=None, wpp=None):
        import hpe
        import torch
        from hpe import _lib, window
        self.hpe, self.torch, self._lib, self.window = hpe, torch, _lib, window
        saved = {k: os.environ.pop(k, None) for k in ("HPE_PSO_FORM", "HPE_PSO_WPP")}
        try:
            if form:
                os.environ["HPE_PSO_FORM"] = form
            if wpp:
                os.environ["HPE_PSO_WPP"] = str(wpp)
            self.hand = make_hand(name)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        self.name = name
        self.ctx = self.hand.ctx
        self.lib = self.ctx.lib
        ub, lb, sd = hpe.reference_bounds()
        self.pso = hpe.PSO()
        self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        self.pso._push(self.ctx)
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        self.radii = np.asarray(self.hand.spheres_radii, dtype=np.float64)
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.h1 = torch.empty((NF, 27), dtype=torch.float64, device="cuda:0")
        self.bufs = {}
        self.slots = {}    # id of a frame list -> first slot
        self.next_slot = 8
        self.sync()

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def start(self):
        x = np.zeros(27)
        x[:26] = self.x0
        return x

    def rule(self, theta, mxy=MXY, mz=MZ):
        S = self.hand.build_hand_model(np.asarray(theta, dtype=np.float64)[:26])
        return self.window.from_spheres(S, self.radii, FOCAL, mxy, mz)

    def slot0(self, frames):
        """The frames device-prepared into slots of this context, once: their first slot."""
        if id(frames) not in self.slots:
            self.slots[id(frames)] = (self.next_slot, frames)  # (the list is kept alive)
            for f, d in enumerate(frames):
                self.ctx.prepare_frame(self.next_slot + f, d)
            self.next_slot += len(frames)
            self.sync()
        return self.slots[id(frames)][0]

    # ---- the single-sequence calls
    def alone(self, kind, frames, refine):
        """prepared / raw: (history n x 27, final state); live: the state after every frame."""
        n = len(frames)
        self.st1.copy_(self.torch.from_numpy(self.start()))
        self.h1.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        if kind == "prepared":
            self.ctx.track_sequence(P, refine, self.st1.data_ptr(), self.slot0(frames), n, K,
                                    self.h1.data_ptr())
        elif kind == "raw":
            raw = self.torch.from_numpy(np.stack(frames)).to("cuda:0")
            self.ctx.track_raw_sequence(P, refine, self.st1.data_ptr(), raw.data_ptr(), n,
                                        frames_per_graph=K, d_hist_ptr=self.h1.data_ptr())
        else:
            out = []
            self.ctx.pipeline_begin(frames[0])
            for f in range(n):
                self.ctx.track_pipelined(P, refine, self.st1.data_ptr(),
                                         frames[f + 1] if f + 1 < n else None)
                self.sync()
                out.append(self.st1.cpu().numpy().copy())
            return np.array(out)
        self.sync()
        return self.h1.cpu().numpy()[:n].copy(), self.st1.cpu().numpy().copy()

    def follow_yard(self, frames):
        """FOLLOW on this context's hand, on the host: frame 0 masked by the rule on x0, frame 1
        too, frame g by the rule on the pipelined loop's state after frame g-2; then the raw
        sequence call on the masked frames."""
        n = len(frames)
        wins = [self.rule(self.x0), self.rule(self.x0)]
        masked = [self.window.apply(frames[g], wins[g]) for g in range(2)]
        self.st1.copy_(self.torch.from_numpy(self.start()))
        self.torch.cuda.synchronize()
        self.ctx.pipeline_begin(masked[0])
        for g in range(n):
            self.ctx.track_pipelined(P, 1, self.st1.data_ptr(), masked[g + 1] if g + 1 < n else None)
            self.sync()
            if g + 2 < n:
                wins.append(self.rule(self.st1.cpu().numpy()))
                masked.append(self.window.apply(frames[g + 2], wins[-1]))
        hist, final = self.alone("raw", masked, 1)
        return dict(wins=wins, masked=masked, hist=hist, final=final)

    # ---- the batch calls
    def bufs_for(self, B, n, tag=None):
        if (B, n, tag) not in self.bufs:
            t = self.torch
            self.bufs[(B, n, tag)] = (t.zeros((B, 27), dtype=t.float64, device="cuda:0"),
                                      t.empty((B, n, 27), dtype=t.float64, device="cuda:0"))
        st, hist = self.bufs[(B, n, tag)]
        st.copy_(self.torch.from_numpy(np.stack([self.start()] * B)))
        hist.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        return st, hist

    def batch(self, kind, lanes, refine, form="auto", tag=None):
        """prepared / raw: (history B x n x 27, states B x 27) over the lanes' frame lists (raw:
        device tensors n x 240 x 320); live: the states after every frame, n x B x 27."""
        B, n = len(lanes), len(lanes[0])
        st, hist = self.bufs_for(B, n, tag)
        self.ctx.set_batch_form(form)
        try:
            if kind == "prepared":
                self.ctx.track_batch(P, refine, st.data_ptr(), [self.slot0(fr) for fr in lanes], n,
                                     K, hist.data_ptr())
            elif kind == "raw":
                self.ctx.track_raw_batch(P, refine, st.data_ptr(), [r.data_ptr() for r in lanes], n,
                                         frames_per_graph=K, d_hist_ptr=hist.data_ptr())
            else:
                out = []
                self.ctx.batch_pipeline_begin([fr[0] for fr in lanes])
                for f in range(n):
                    self.ctx.track_batch_pipelined(P, refine, st.data_ptr(),
                                                   [fr[f + 1] for fr in lanes] if f + 1 < n else None)
                    self.sync()
                    out.append(st.cpu().numpy().copy())
                return np.array(out)
            self.sync()
        finally:
            self.ctx.set_batch_form("auto")
        return hist.cpu().numpy(), st.cpu().numpy()


class Pool:
    def __init__(self):
        self.envs = {}
        self.frames = {}   # (hand, seed) -> NF frames rendered by the hand's yardstick context
        self.raws = {}
        self.yards = {}    # computed once, shared, never changed
        self.batch_env = Env("A")  # the context under test: created with A, never a yardstick

    def env(self, name, form=None, wpp=None):
        if (name, form, wpp) not in self.envs:
            self.envs[(name, form, wpp)] = Env(name, form, wpp)
        return self.envs[(name, form, wpp)]

    def stream(self, name, seed=None):
        from hpe import synth
        seed = SEED[name] if seed is None else seed
        if (name, seed) not in self.frames:
            ctx = self.env(name).ctx
            self.frames[(name, seed)] = [np.ascontiguousarray(ctx.render_depth(th), dtype=np.float32)
                                         for th in synth.trajectory(NF, seed)]
        return self.frames[(name, seed)]

    def raw(self, name, seed=None):
        fr = self.stream(name, seed)
        if id(fr) not in self.raws:
            import torch
            self.raws[id(fr)] = torch.from_numpy(np.stack(fr)).to("cuda:0")
        return self.raws[id(fr)]

    def lanes(self, kind, names, n=NF):
        if kind == "raw":
            return [self.raw(h)[:n] for h in names]
        return [self.stream(h)[:n] if n != NF else self.stream(h) for h in names]

    def yard(self, name, kind, refine, n=NF, frames_of=None, form=None, wpp=None):
        """The single-sequence call of hand `name`'s own context on the frames of hand
        `frames_of` (default: its own)."""
        key = (name, kind, refine, n, frames_of, form, wpp)
        if key not in self.yards:
            fr = self.stream(frames_of or name)
            self.yards[key] = self.env(name, form, wpp).alone(kind, fr if n == NF else fr[:n], refine)
        return self.yards[key]

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
    yield pool.batch_env
    try:
        pool.batch_env.ctx.set_batch_hands(None)
    except pool.batch_env.hpe.HpeError:
        pass  # a live batch a failed test left behind keeps its hands


def check(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


# ---- 1. a second hand is right at all: FK and costs of the S and L contexts against the oracle
@pytest.mark.parametrize("name", ["S", "L"])
def test_scaled_hand_against_the_oracle(pool, oracle, name):
    import hand_data
    import hpe
    import oracle_np
    s, rs = SCALES[name]
    geo, rad = hand_data.geometry_cm()
    ora = oracle.hand(geo * s, rad * rs)
    nph = oracle_np.Hand(geo * s, rad * rs)
    hand = pool.env(name).hand
    rng = np.random.default_rng(11)
    th = np.vstack([oracle_np.X0, hand_data.random_thetas(rng, 15, spread=3.0)])
    S, J = hand.build_batch(th)
    for i in range(len(th)):
        Sr, Jr = oracle.build(ora, th[i], joints=True)
        np.testing.assert_allclose(S[i], Sr, rtol=0, atol=1e-9)
        np.testing.assert_allclose(J[i], Jr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(S[0], nph.build_hand_model(th[0]), rtol=0, atol=1e-9)
    # not the reference hand's centres
    Sa, _ = pool.env("A").hand.build_batch(th[:1])
    assert np.abs(S[0] - Sa[0]).max() > 0.1
    truth = hand_data.trajectory(3, seed=5)[2]
    d = oracle_np.render_depth_mm(nph, truth)
    obs = oracle.preprocess(d, downsample=True)
    om = hpe.observedmodel()
    om.to_cm, om.downsample, om.focal_len = True, True, FOCAL
    om.set_depth_mm(d)
    cf = hpe.costfunc(hand, om)
    tc = hand_data.random_thetas(rng, 16, x0=truth, spread=0.4)
    tc[0] = truth
    for coll in (False, True):
        np.testing.assert_allclose(cf.cal_cost_batch(tc, with_collision=coll),
                                   oracle.eval_costs(ora, obs, tc, with_collision=coll),
                                   rtol=1e-9, atol=0)


# ---- 2. prepared, raw and live batch, hands [A, S, L]
@pytest.mark.parametrize("refine", [1, 0])
@pytest.mark.parametrize("kind", ["prepared", "raw", "live"])
def test_three_hands(pool, env, kind, refine):
    names = ["A", "S", "L"]
    yards = [pool.yard(h, kind, refine) for h in names]
    pool.set_hands(env, names)
    got = env.batch(kind, pool.lanes(kind, names), refine)
    for b, h in enumerate(names):
        if kind == "live":
            for f in range(NF):  # after every frame
                assert np.array_equal(got[f, b], yards[b][f]), (h, f)
        else:
            check((got[0][b], got[1][b]), yards[b], h)
    assert np.isfinite(got if kind == "live" else got[0]).all()
    # the hand matters: on the same frames (A's) the three yardsticks differ from one another
    same = [pool.yard(h, kind, refine, frames_of="A") for h in names]
    hist = [y if kind == "live" else y[0] for y in same]
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.array_equal(hist[i], hist[j]), (names[i], names[j])


# ---- 3. indexing ends
@pytest.mark.parametrize("odd", [15, 0])
def test_sixteen_lanes_one_odd_hand(pool, env, odd):
    names = ["A"] * 16
    names[odd] = "S"
    ya, ys = pool.yard("A", "raw", 1, n=2), pool.yard("S", "raw", 1, n=2)
    pool.set_hands(env, names)
    hist, st = env.batch("raw", pool.lanes("raw", names, 2), 1)
    for b, h in enumerate(names):
        check((hist[b], st[b]), ys if h == "S" else ya, (b, h))
    assert not np.array_equal(hist[odd], hist[1])


def test_permuted_hands(pool, env):
    names = ["L", "A", "S"]
    pool.set_hands(env, names)
    hist, st = env.batch("raw", pool.lanes("raw", names), 1)
    for b, h in enumerate(names):
        check((hist[b], st[b]), pool.yard(h, "raw", 1), (b, h))


# ---- 4. the wave form, one hand per workgroup
@pytest.mark.parametrize("kind,wpp", [("raw", 2), ("raw", 1), ("live", 2)])
def test_wave_form(pool, kind, wpp):
    """The wave form's final kernels evaluate cal_cost(bestp) themselves (same_eval = 0), so
    these cases are the ones that see the hand the final kernel of a raw and of a live batch
    stages."""
    names = ["S", "V"]
    # P = 32, B = 2: two waves per particle on a default context; one on a context that forces it
    benv = pool.batch_env if wpp == 2 else pool.env("A", None, 1)
    assert benv.ctx.batch_wave_wpp(P, 2) == wpp
    yards = [pool.yard(h, kind, 1, form="wave", wpp=wpp) for h in names]
    pool.set_hands(benv, names)
    try:
        got = benv.batch(kind, pool.lanes(kind, names), 1, form="wave")
    finally:
        benv.ctx.set_batch_hands(None)
    for b, h in enumerate(names):
        if kind == "live":
            for f in range(NF):
                assert np.array_equal(got[f, b], yards[b][f]), (h, f, wpp)
        else:
            check((got[0][b], got[1][b]), yards[b], (h, wpp))
    assert np.isfinite(got if kind == "live" else got[0]).all()
    other = pool.yard("V", kind, 1, frames_of="S", form="wave", wpp=wpp)
    assert not np.array_equal(yards[0] if kind == "live" else yards[0][0],
                              other if kind == "live" else other[0])


# ---- 5. FOLLOW windows from the lane's own hand
def test_follow_windows_with_lane_hands(pool, env):
    names = ["S", "L"]
    yards = [pool.env(h).follow_yard(pool.stream(h)) for h in names]
    own = [pool.env(h).ctx.window_from_pose(env.x0, FOCAL, MXY, MZ) for h in names]
    # no lane hands: the lane call is hpe_window_from_pose, field for field
    for lane in (0, 1, 15):
        assert env.ctx.lane_window_from_pose(lane, env.x0, FOCAL, MXY, MZ) == \
            env.ctx.window_from_pose(env.x0, FOCAL, MXY, MZ)
    pool.set_hands(env, names)
    init = [env.ctx.lane_window_from_pose(b, env.x0, FOCAL, MXY, MZ) for b in range(2)]
    for b in range(2):
        assert init[b] == own[b] == yards[b]["wins"][0], b
    assert init[0] != init[1] and init[0] != env.ctx.window_from_pose(env.x0, FOCAL, MXY, MZ)
    env.ctx.set_batch_window("follow", init, MXY, MZ)
    try:
        hist, st = env.batch("raw", pool.lanes("raw", names), 1)
        tables = [env.ctx.batch_windows_readback(p, 2) for p in (0, 1)]
    finally:
        env.ctx.set_batch_window("off")
    for b, y in enumerate(yards):
        check((hist[b], st[b]), (y["hist"], y["final"]), names[b])
        # frame g was prepared into parity g & 1 through the window of the host rule
        assert tables[(NF - 1) & 1][b] == y["wins"][NF - 1], b
        assert tables[(NF - 2) & 1][b] == y["wins"][NF - 2], b
        assert not any(env.window.is_whole(w) for w in y["wins"])
        assert any(w != y["wins"][0] for w in y["wins"][2:])
    assert np.isfinite(hist).all()


# ---- 6. graphs hold the table's address alone
def test_hands_change_without_a_capture(pool, env):
    yards = {h: pool.yard(h, "raw", 1) for h in "ASL"}

    def run(names, hands):
        pool.set_hands(env, hands)
        return env.batch("raw", pool.lanes("raw", names), 1, tag="graphs")

    plain = run(["A", "A"], None)
    first = run(["A", "S"], ["A", "S"])
    c = env.ctx.graph_captures()
    second = run(["L", "A"], ["L", "A"])
    assert env.ctx.graph_captures() == c
    again = run(["A", "A"], None)
    assert env.ctx.graph_captures() == c
    for b, h in enumerate("AS"):
        check((first[0][b], first[1][b]), yards[h], h)
    for b, h in enumerate("LA"):
        check((second[0][b], second[1][b]), yards[h], h)
    check(again, plain, "hands = NULL")
    check((plain[0][0], plain[1][0]), yards["A"], "no hands")


# ---- 7. the lane hands never leak into the single-sequence calls
def test_no_leak(pool, env):
    fr = pool.stream("A")
    th = np.vstack([env.x0, env.x0 + 2.0])
    before = (env.alone("prepared", fr, 1), env.hand.build_batch(th),
              env.ctx.window_from_pose(env.x0, FOCAL, MXY, MZ))
    pool.set_hands(env, ["S", "L"])
    after = (env.alone("prepared", fr, 1), env.hand.build_batch(th),
             env.ctx.window_from_pose(env.x0, FOCAL, MXY, MZ))
    check(after[0], before[0], "track_sequence")
    check(after[1], before[1], "build_spheres")
    assert after[2] == before[2]
    # hands = NULL: a batch equals the batch of a context that never called the function
    pool.set_hands(env, None)
    names = ["A", "A"]
    got = env.batch("raw", pool.lanes("raw", names), 1)
    fresh = pool.env("A").batch("raw", pool.lanes("raw", names), 1)
    check(got, fresh, "hands = NULL")


# ---- 8. refusals change nothing
def test_refusals_change_nothing(pool, env):
    _lib, lib, h = env._lib, env.lib, env.ctx.h
    M = _lib.BATCH_MAX
    names = ["S", "L"]
    lanes = pool.lanes("raw", names)
    want = [pool.yard(n, "raw", 1) for n in names]
    live_want = [pool.yard(n, "live", 1) for n in names]

    def err():
        return lib.hpe_last_error(h)

    def params(n):
        p = _lib.HandParams()
        C.memmove(C.byref(p), C.byref(pool.env(n).hand.params), C.sizeof(p))
        return p

    def still():
        hist, st = env.batch("raw", lanes, 1)
        for b in range(2):
            check((hist[b], st[b]), want[b], names[b])

    pool.set_hands(env, names)
    still()
    arr = (_lib.HandParams * (M + 1))(*[params("A") for _ in range(M + 1)])
    bad = params("A")
    bad.fg_spheres[0] = 3
    arr[1] = bad
    assert lib.hpe_set_batch_hands(h, 2, arr) == _lib.HPE_E_ARG and b"sphere counts" in err()
    still()
    bad = params("A")
    bad.tb_spheres[3] = 1
    arr[1] = bad
    assert lib.hpe_set_batch_hands(h, 2, arr) == _lib.HPE_E_ARG and b"sphere counts" in err()
    bad = params("A")
    bad.geo_cm[7] = float("nan")
    arr[1] = bad
    assert lib.hpe_set_batch_hands(h, 2, arr) == _lib.HPE_E_ARG and b"finite" in err()
    still()
    arr[1] = params("A")
    for B in (0, M + 1):
        assert lib.hpe_set_batch_hands(h, B, arr) == _lib.HPE_E_ARG and b"lanes" in err()
    still()
    assert lib.hpe_set_batch_hands(None, 2, arr) == _lib.HPE_E_ARG
    # a batch call or begin with another lane count than the hands'
    st = env.torch.zeros((3, 27), dtype=env.torch.float64, device="cuda:0")
    st[:, :26] = env.torch.from_numpy(env.x0)
    env.torch.cuda.synchronize()
    raws3 = (C.c_void_p * 3)(*[pool.raw("A").data_ptr()] * 3)
    assert lib.hpe_track_raw_batch_dev(h, P, 1, 3, C.c_void_p(st.data_ptr()), raws3, NF, 1, 1, FOCAL,
                                       K, None) == _lib.HPE_E_ARG and b"hands were set for 2" in err()
    s0 = env.slot0(pool.stream("A"))
    slots3 = (C.c_int32 * 3)(s0, s0, s0)
    assert lib.hpe_track_batch_dev(h, P, 1, 3, C.c_void_p(st.data_ptr()), slots3, NF, K,
                                   None) == _lib.HPE_E_ARG and b"hands were set for 2" in err()
    f0 = pool.stream("A")[0]
    fr3 = (C.c_void_p * 3)(*[f0.ctypes.data] * 3)
    assert lib.hpe_batch_pipeline_begin(h, 3, fr3, 1, 1, FOCAL) == _lib.HPE_E_ARG
    assert b"hands were set for 2" in err()
    still()
    # lanes outside 0..15 of hpe_lane_window_from_pose
    w = _lib.Window(1, 2, 3, 4, 5.0, 6.0)
    th = env.x0.ctypes.data_as(_lib.dp)
    for lane in (-1, M):
        assert lib.hpe_lane_window_from_pose(h, lane, th, FOCAL, MXY, MZ, C.byref(w)) == _lib.HPE_E_ARG
        assert b"lane" in err()
    assert lib.hpe_lane_window_from_pose(None, 0, th, FOCAL, MXY, MZ, C.byref(w)) == _lib.HPE_E_ARG
    assert env.window.as_window(w) == (1, 2, 3, 4, 5.0, 6.0)
    still()
    # a live batch in progress keeps the hands it began with: every set is refused, NULL included
    fr = pool.lanes("live", names)
    st2 = env.torch.zeros((2, 27), dtype=env.torch.float64, device="cuda:0")
    st2[:, :26] = env.torch.from_numpy(env.x0)
    env.torch.cuda.synchronize()
    env.ctx.batch_pipeline_begin([f[0] for f in fr])
    assert lib.hpe_set_batch_hands(h, 2, arr) == _lib.HPE_E_STATE and b"live batch" in err()
    assert lib.hpe_set_batch_hands(h, 0, None) == _lib.HPE_E_STATE and b"live batch" in err()
    for f in range(NF):
        env.ctx.track_batch_pipelined(P, 1, st2.data_ptr(), [x[f + 1] for x in fr] if f + 1 < NF else None)
        env.sync()
        got = st2.cpu().numpy()
        for b in range(2):
            assert np.array_equal(got[b], live_want[b][f]), (f, b)
    still()
    assert lib.hpe_set_batch_hands(h, 0, None) == 0  # the batch has ended
