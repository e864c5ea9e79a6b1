"""Lane input of the live batch: 16-bit frames read as such by the device
(hpe_batch_pipeline_begin_u16 / hpe_track_batch_pipelined_u16) and the lanes' pinned buffers filled
in place (hpe_batch_frame_buffer).

The yardstick is always the single pipelined loop (hpe_pipeline_begin + hpe_track_pipelined) of
one stream alone on frames converted on the host by hpe.depth_u16_to_mm, compared with
np.array_equal on the 27-double state after EVERY frame; never a batch.

Two quantisations of the rendered frames:
  Q1   np.rint(render) at unit 1.0 -- a millimetre camera;
  Qhi  np.rint(render / float32(0.0055)) at unit float32(0.0055): every non-zero pixel lies in
       [32768, 65535] (asserted on the inputs), so a sign-extending 16-bit load, silent on Q1,
       reads negative depths, and a dropped unit multiply reads metres-deep ones.

Small shapes: P = 64, maxiter 7 (G = 6), at most 6 frames per lane (hpe.synth.trajectory seeds 0, 1,
2 rendered with render_depth), at most 3 lanes.  One context runs every batch but the two capture
counts, which take a context of their own (a cache shared with the other tests could be emptied
between the two runs compared); the wave-form and lane-hand yardsticks need the contexts those
features define them on (tests/test_gpu_batch_wave.py, tests/test_gpu_batch_hands.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF = 64, 7, 6
FOCAL, MXY, MZ = 241.42, 1.0, 2.0
UHI = np.float32(0.0055)
QUANT = {"Q1": np.float32(1.0), "Qhi": UHI, "Qhalf": np.float32(0.5)}


def quantise(render, unit):
    """The 16-bit frame of a rendered float mm frame at `unit` mm per count (0 stays 0)."""
    q = np.rint(np.asarray(render, dtype=np.float32) / np.float32(unit))
    assert q.min() >= 0 and q.max() <= 65535
    return np.ascontiguousarray(q.astype(np.uint16))


class Env:
    """One context on hand `hand` (default: the reference hand; created under HPE_PSO_FORM /
    HPE_PSO_WPP if given) with the single pipelined loop -- the yardstick -- and the live batch."""

    def __init__(self, hand=None, form=None, wpp=None):
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
            self.hand = hpe.reference_hand(device=0) if hand is None else hpe.scaled_hand(*hand)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        self.ctx = self.hand.ctx
        self.lib = self.ctx.lib
        ub, lb, sd = hpe.reference_bounds()
        self.pso = hpe.PSO()
        self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        self.pso._push(self.ctx)
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        self.radii = np.asarray(self.hand.spheres_radii, dtype=np.float64)
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.states = {}
        self._single = {}  # yardsticks: computed once, shared, never changed
        # before any begin on this context: the refusal test reads this
        buf = C.c_void_p()
        self.rc_buffer_before_begin = self.lib.hpe_batch_frame_buffer(self.ctx.h, 0, C.byref(buf), None)
        self.sync()

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def err(self):
        return self.lib.hpe_last_error(self.ctx.h).decode()

    def start(self, x0=None):
        x = np.zeros(27)
        x[:26] = self.x0 if x0 is None else np.asarray(x0)[:26]
        return x

    def rule(self, theta):
        S = self.hand.build_hand_model(np.asarray(theta, dtype=np.float64)[:26])
        return self.window.from_spheres(S, self.radii, FOCAL, MXY, MZ)

    def loop(self, frames, refine, x0=None):
        """The single pipelined loop over float frames: the state after every frame."""
        n = len(frames)
        self.st1.copy_(self.torch.from_numpy(self.start(x0)))
        self.torch.cuda.synchronize()
        out = []
        self.ctx.pipeline_begin(frames[0])
        for f in range(n):
            self.ctx.track_pipelined(P, refine, self.st1.data_ptr(), frames[f + 1] if f + 1 < n else None)
            self.sync()
            out.append(self.st1.cpu().numpy().copy())
        return np.array(out)

    def single(self, key, frames, refine):
        key = (key, len(frames), refine)
        if key not in self._single:
            self._single[key] = self.loop(frames, refine)
        return self._single[key]

    def batch_states(self, B, tag=None):
        if (B, tag) not in self.states:
            self.states[(B, tag)] = self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0")
        return self.states[(B, tag)]

    def live(self, lanes, refine, input="u16", unit=1.0, in_place=(), x0s=None, tag=None):
        """The live batch over the lanes' frame lists (all of one length n), a frame per lane and
        call: the states after every frame (n x B x 27).  in_place: the lanes whose next frames
        are written into batch_frame_buffer's view and passed back as that view."""
        B, n = len(lanes), len(lanes[0])
        st = self.batch_states(B, tag)
        st.copy_(self.torch.from_numpy(np.stack([self.start(None if x0s is None else x0s[b])
                                                 for b in range(B)])))
        self.torch.cuda.synchronize()
        out = []
        self.ctx.batch_pipeline_begin([fr[0].copy() for fr in lanes], input=input, unit_mm=unit)
        for f in range(n):
            nxt = None
            if f + 1 < n:
                nxt = []
                for b, fr in enumerate(lanes):
                    if b in in_place:
                        buf = self.ctx.batch_frame_buffer(b)
                        assert buf.dtype == fr[f + 1].dtype and buf.shape == (240, 320)
                        buf[:] = fr[f + 1]
                        nxt.append(buf)
                    else:
                        nxt.append(fr[f + 1].copy())
            self.ctx.track_batch_pipelined(P, refine, st.data_ptr(), nxt)
            self.sync()
            out.append(st.cpu().numpy().copy())
        return np.array(out)


class Pool:
    def __init__(self):
        from hpe import synth
        self.env = Env()
        e = self.env
        self.render = {s: [np.ascontiguousarray(e.ctx.render_depth(th), dtype=np.float32)
                           for th in synth.trajectory(NF, s)] for s in range(3)}
        self.q, self.f = {}, {}  # (quantisation, stream) -> the u16 frames / their float conversion
        for name, unit in QUANT.items():
            for s in range(3):
                self.add((name, s), self.render[s], unit)
        self.others = {}

    def add(self, key, renders, unit):
        self.q[key] = [quantise(r, unit) for r in renders]
        self.f[key] = [self.env.hpe.depth_u16_to_mm(q, unit) for q in self.q[key]]
        if key[0] == "Qhi":  # the inputs are what the case needs: every depth above 32767
            for q in self.q[key]:
                nz = q[q != 0]
                assert nz.size and nz.min() >= 32768 and nz.max() <= 65535

    def other(self, key, **kw):
        if key not in self.others:
            self.others[key] = Env(**kw)
        return self.others[key]

    def close(self):
        self.env.ctx.close()
        for e in self.others.values():
            e.ctx.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


@pytest.fixture(scope="module")
def env(pool):
    return pool.env


def check_lanes(pool, env, keys, n, refine, yard=None, equal_nan=False, **kw):
    """The u16 live batch over the (quantisation, stream) keys against each lane's yardstick."""
    unit = QUANT[keys[0][0]]
    got = env.live([pool.q[k][:n] for k in keys], refine, "u16", unit, **kw)
    for b, k in enumerate(keys):
        want = (yard or env).single(k, pool.f[k][:n], refine)
        for f in range(n):
            assert np.array_equal(got[f, b], want[f], equal_nan=equal_nan), (k, b, f)
    return got


# ---- 1. both quantisations, refine on and off
@pytest.mark.parametrize("refine", [1, 0])
@pytest.mark.parametrize("quant", ["Q1", "Qhi"])
def test_three_lanes_five_frames(pool, env, quant, refine):
    got = check_lanes(pool, env, [(quant, s) for s in range(3)], 5, refine)
    assert np.isfinite(got).all()
    assert not np.array_equal(got[:, 0], got[:, 1])
    # the quantised stream is not the rendered one: the yardstick is on the converted frames
    assert any(not np.array_equal(a, b) for a, b in zip(pool.f[(quant, 0)], pool.render[0]))


# ---- 2. Qhi behind windows
def test_fixed_windows(pool, env):
    W = env.window
    w = env.rule(env.x0)
    half = W.Window(w.row_lo, w.row_hi, w.col_lo, (w.col_lo + w.col_hi) // 2, w.z_lo, w.z_hi)
    wins = [half, W.WHOLE]
    keys = [("Qhi", 0), ("Qhi", 1)]
    n = 4
    kept = np.count_nonzero(W.apply(pool.f[keys[0]][0], half))
    assert 0 < kept < np.count_nonzero(pool.f[keys[0]][0])  # it does cut the hand
    env.ctx.set_batch_window("fixed", wins, MXY, MZ)
    try:
        got = env.live([pool.q[k][:n] for k in keys], 1, "u16", UHI)
    finally:
        env.ctx.set_batch_window("off")
    for b, k in enumerate(keys):
        want = env.single(("fixed", k, tuple(wins[b])), [W.apply(f, wins[b]) for f in pool.f[k][:n]], 1)
        for f in range(n):
            assert np.array_equal(got[f, b], want[f]), (b, f)
    assert not np.array_equal(got[:, 0], env.single(keys[0], pool.f[keys[0]][:n], 1))


def follow_yard(env, frames, x0, init):
    """FOLLOW's yardstick, step by step with the single pipelined loop (as
    tests/test_gpu_batch_window.py builds it): frame 0 masked by init, frame 1 by the pose rule
    on x0, frame g by the rule on the loop's state after frame g-2.  (masked frames, states)."""
    W, n = env.window, len(frames)
    wins = [W.as_window(init), env.rule(x0)]
    masked = [W.apply(frames[g], wins[g]) for g in range(min(n, 2))]
    env.st1.copy_(env.torch.from_numpy(env.start(x0)))
    env.torch.cuda.synchronize()
    states = []
    env.ctx.pipeline_begin(masked[0])
    for g in range(n):
        env.ctx.track_pipelined(P, 1, env.st1.data_ptr(), masked[g + 1] if g + 1 < n else None)
        env.sync()
        states.append(env.st1.cpu().numpy().copy())
        if g + 2 < n:
            wins.append(env.rule(states[g]))
            masked.append(W.apply(frames[g + 2], wins[-1]))
    return masked, np.array(states)


@pytest.mark.parametrize("case", ["two streams", "two hands in one buffer"])
def test_follow_windows(pool, env, case):
    from hpe import synth
    n = 4
    if case == "two streams":
        x0s = [env.x0, env.x0]
        lanes_q = [pool.q[("Qhi", 0)][:n], pool.q[("Qhi", 1)][:n]]
        lanes_f = [pool.f[("Qhi", 0)][:n], pool.f[("Qhi", 1)][:n]]
    else:  # both lanes read one buffer that holds two hands, each through its own window
        d = 9.0
        poses = [synth.trajectory(n, 0), synth.trajectory(n, 1)]
        x0s = [env.x0.copy(), env.x0.copy()]
        for lane, sign in ((0, -1.0), (1, 1.0)):
            poses[lane][:, 3] += sign * d
            x0s[lane][3] += sign * d
        renders = []
        for f in range(n):
            a = env.ctx.render_depth(poses[0][f])
            b = env.ctx.render_depth(poses[1][f])
            renders.append(np.where((a > 0) & (b > 0), np.minimum(a, b), a + b).astype(np.float32))
        pool.add(("Qhi", "two hands"), renders, UHI)
        lanes_q = [pool.q[("Qhi", "two hands")]] * 2
        lanes_f = [pool.f[("Qhi", "two hands")]] * 2
    inits = [env.rule(x) for x in x0s]
    yards = [follow_yard(env, lanes_f[b], x0s[b], inits[b]) for b in range(2)]
    for b in range(2):  # every mask keeps some of the frame and, with two hands, removes some
        for g in range(n):
            kept = np.count_nonzero(yards[b][0][g])
            assert 0 < kept <= np.count_nonzero(lanes_f[b][g])
            if case != "two streams":
                assert kept < np.count_nonzero(lanes_f[b][g])
    env.ctx.set_batch_window("follow", inits, MXY, MZ)
    try:
        got = env.live(lanes_q, 1, "u16", UHI, x0s=x0s)
    finally:
        env.ctx.set_batch_window("off")
    for b in range(2):
        for f in range(n):
            assert np.array_equal(got[f, b], yards[b][1][f]), (b, f)
    assert np.isfinite(got).all()


# ---- 3. free pacing: a lane that starts empty, a lane that skips a call
def test_free_pacing(pool, env):
    torch = env.torch
    keys = [("Q1", s) for s in range(3)]
    # the lanes given a frame at the begin and by every call (None: the last call)
    sched = [{0, 1}, {0, 2}, {0, 1, 2}, {0, 1, 2}, None]
    st = env.batch_states(3, "paced")
    x = np.stack([env.start(), env.start(), np.full(27, np.nan)])
    st.copy_(torch.from_numpy(x))
    torch.cuda.synchronize()
    took = [0, 0, 0]
    tracked = [[], [], []]

    def frames(step):
        if step is None:
            return None
        fr = [None] * 3
        for b in step:
            fr[b] = pool.q[keys[b]][took[b]].copy()
            took[b] += 1
        return fr

    env.ctx.set_batch_pacing("free")
    try:
        env.ctx.batch_pipeline_begin(frames(sched[0]), input="u16", unit_mm=1.0)
        for k in range(len(sched) - 1):
            pending = sched[k]
            if k == 1:  # lane 2 joined: its row just before the call that tracks its first frame
                st[2].copy_(torch.from_numpy(env.start()))
                torch.cuda.synchronize()
            prev = st.cpu().numpy().copy()
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), frames(sched[k + 1]))
            env.sync()
            now = st.cpu().numpy().copy()
            for b in range(3):
                if b in pending:
                    tracked[b].append(now[b])
                else:  # idle: bit for bit what it was, the NaN row included
                    assert np.array_equal(now[b].view(np.uint64), prev[b].view(np.uint64)), (b, k)
    finally:
        env.sync()
        env.ctx.set_batch_pacing("lockstep")
    assert [len(t) for t in tracked] == [4, 3, 3] == took
    for b, k in enumerate(keys):
        want = env.single(k, pool.f[k][:took[b]], 1)
        for f in range(took[b]):
            assert np.array_equal(tracked[b][f], want[f]), (b, f)


# ---- 4. the wave form
def test_wave_form(pool, env):
    keys = [("Q1", 1), ("Q1", 2)]
    wpp = env.ctx.batch_wave_wpp(P, 2)
    assert wpp in (1, 2)
    yard = pool.other(("wave", wpp), form="wave", wpp=wpp)
    env.ctx.set_batch_form("wave")
    try:
        got = check_lanes(pool, env, keys, 3, 1, yard=yard, tag="wave")
    finally:
        env.ctx.set_batch_form("auto")
    assert np.isfinite(got).all()


# ---- 5. lane hands
def test_lane_hands(pool, env):
    scales = [(0.9, 0.85), (1.1, 1.2)]
    keys = [("Q1", 1), ("Q1", 2)]
    yards = [pool.other(("hand", s), hand=s) for s in scales]
    env.ctx.set_batch_hands([y.hand for y in yards])
    try:
        got = env.live([pool.q[k][:3] for k in keys], 1, "u16", 1.0, tag="hands")
    finally:
        env.ctx.set_batch_hands(None)
    for b, k in enumerate(keys):
        want = yards[b].single(k, pool.f[k][:3], 1)
        for f in range(3):
            assert np.array_equal(got[f, b], want[f]), (b, f)
        assert not np.array_equal(got[:, b], env.single(k, pool.f[k][:3], 1))


# ---- 6. an all-zero frame in the middle of a stream
def test_all_zero_frame(pool, env):
    hole_q = [q.copy() for q in pool.q[("Q1", 0)][:4]]
    hole_q[1][:] = 0
    pool.q[("Q1", "hole")] = hole_q
    pool.f[("Q1", "hole")] = [env.hpe.depth_u16_to_mm(q, 1.0) for q in hole_q]
    assert not pool.f[("Q1", "hole")][1].any()
    got = check_lanes(pool, env, [("Q1", "hole"), ("Q1", 1)], 4, 1, equal_nan=True)
    assert np.isfinite(got[:, 1]).all()


# ---- 7. in place
@pytest.mark.parametrize("input", ["f32", "u16"])
def test_in_place(pool, env, input):
    keys = [("Q1", s) for s in range(3)]
    src = pool.q if input == "u16" else pool.f
    lanes = [src[k][:5] for k in keys]
    want = [env.single(k, pool.f[k][:5], 1) for k in keys]
    for in_place in ({0, 1, 2}, {0}):  # every lane; lane 0 alone beside two ordinary arrays
        got = env.live(lanes, 1, input, 1.0, in_place=in_place)
        for b in range(3):
            for f in range(5):
                assert np.array_equal(got[f, b], want[b][f]), (in_place, b, f)


@pytest.mark.parametrize("input", ["f32", "u16"])
def test_in_place_replays_the_copying_graphs(pool, input):
    own = pool.other("captures")
    keys = [("Q1", s) for s in range(3)]
    src = pool.q if input == "u16" else pool.f
    lanes = [src[k][:5] for k in keys]
    c0 = own.ctx.graph_captures()
    a = own.live(lanes, 1, input, 1.0, tag=input)
    c1 = own.ctx.graph_captures()
    b = own.live(lanes, 1, input, 1.0, in_place={0, 1, 2}, tag=input)
    c2 = own.ctx.graph_captures()
    assert 1 <= c1 - c0 <= 3  # parities 0 and 1 with a next frame, one without
    assert c2 == c1  # nothing captured: the in-place calls replayed the copying calls' graphs
    assert np.array_equal(a, b)


def test_stale_buffer_is_refused_and_the_batch_goes_on(pool, env):
    _lib = env._lib
    keys = [("Q1", 0), ("Q1", 1)]
    n = 4
    st = env.batch_states(2)
    st.copy_(env.torch.from_numpy(np.stack([env.start(), env.start()])))
    env.torch.cuda.synchronize()
    env.ctx.batch_pipeline_begin([pool.q[k][0] for k in keys], input="u16", unit_mm=1.0)
    out, old = [], None
    for f in range(n):
        nxt = None
        if f + 1 < n:
            bufs = [env.ctx.batch_frame_buffer(b) for b in range(2)]
            again = [env.ctx.batch_frame_buffer(b) for b in range(2)]
            for b in range(2):  # asking twice gives the same memory; the lanes' buffers differ
                assert again[b].ctypes.data == bufs[b].ctypes.data
                bufs[b][:] = pool.q[keys[b]][f + 1]
            assert bufs[0].ctypes.data != bufs[1].ctypes.data
            if old is not None:  # the previous call's pointer: its frame is current now
                assert old[0].ctypes.data != bufs[0].ctypes.data
                before = st.cpu().numpy().copy()
                arr = (C.c_void_p * 2)(old[0].ctypes.data, bufs[1].ctypes.data)
                rc = env.lib.hpe_track_batch_pipelined_u16(env.ctx.h, P, 1, 2,
                                                           C.c_void_p(st.data_ptr()), arr)
                assert rc == _lib.HPE_E_ARG and "stale frame buffer" in env.err()
                env.sync()
                assert np.array_equal(st.cpu().numpy(), before)  # nothing ran
            nxt = old = bufs
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), nxt)
        env.sync()
        out.append(st.cpu().numpy().copy())
    for b, k in enumerate(keys):
        want = env.single(k, pool.f[k][:n], 1)
        for f in range(n):
            assert np.array_equal(out[f][b], want[f]), (b, f)


# ---- 8. format and unit
def test_a_batch_keeps_its_format(pool, env):
    _lib, lib, h = env._lib, env.lib, env.ctx.h
    st = env.batch_states(1)
    st.copy_(env.torch.from_numpy(env.start()[None]))
    env.torch.cuda.synchronize()
    q, f = pool.q[("Q1", 0)], pool.f[("Q1", 0)]
    fa = (C.c_void_p * 1)(f[1].ctypes.data)
    qa = (C.c_void_p * 1)(q[1].ctypes.data)
    sp = C.c_void_p(st.data_ptr())
    env.ctx.batch_pipeline_begin([q[0]], input="u16", unit_mm=1.0)
    assert lib.hpe_track_batch_pipelined(h, P, 1, 1, sp, fa) == _lib.HPE_E_STATE
    assert "u16" in env.err() and "f32" in env.err()
    assert lib.hpe_track_batch_pipelined(h, P, 1, 1, sp, None) == _lib.HPE_E_STATE
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)  # the batch is alive: this ends it
    env.sync()
    assert np.array_equal(st.cpu().numpy()[0], env.single(("Q1", 0), f[:1], 1)[0])
    st.copy_(env.torch.from_numpy(env.start()[None]))
    env.torch.cuda.synchronize()
    env.ctx.batch_pipeline_begin([f[0]])
    assert lib.hpe_track_batch_pipelined_u16(h, P, 1, 1, sp, qa) == _lib.HPE_E_STATE
    assert "u16" in env.err() and "f32" in env.err()
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)
    env.sync()
    assert np.array_equal(st.cpu().numpy()[0], env.single(("Q1", 0), f[:1], 1)[0])


@pytest.mark.parametrize("unit", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_bad_unit(pool, env, unit):
    qa = (C.c_void_p * 1)(pool.q[("Q1", 0)][0].ctypes.data)
    rc = env.lib.hpe_batch_pipeline_begin_u16(env.ctx.h, 1, qa, unit, 1, 1, FOCAL)
    assert rc == env._lib.HPE_E_ARG and "unit" in env.err()


def test_frame_buffer_refusals(pool, env):
    _lib, lib, h = env._lib, env.lib, env.ctx.h
    assert env.rc_buffer_before_begin == _lib.HPE_E_STATE
    buf, nb = C.c_void_p(), C.c_size_t(0)
    st = env.batch_states(2)
    env.ctx.batch_pipeline_begin([pool.q[("Q1", 0)][0]] * 2, input="u16", unit_mm=1.0)
    assert lib.hpe_batch_frame_buffer(h, 2, C.byref(buf), None) == _lib.HPE_E_ARG
    assert lib.hpe_batch_frame_buffer(h, -1, C.byref(buf), None) == _lib.HPE_E_ARG
    assert lib.hpe_batch_frame_buffer(h, 0, None, C.byref(nb)) == _lib.HPE_E_ARG
    assert lib.hpe_batch_frame_buffer(h, 1, C.byref(buf), C.byref(nb)) == 0
    assert buf.value and nb.value == 2 * 240 * 320
    st.copy_(env.torch.from_numpy(np.stack([env.start(), env.start()])))
    env.torch.cuda.synchronize()
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)
    env.sync()
    assert lib.hpe_batch_frame_buffer(h, 0, C.byref(buf), None) == _lib.HPE_E_STATE  # it ended
    env.ctx.batch_pipeline_begin([pool.f[("Q1", 0)][0]])
    assert lib.hpe_batch_frame_buffer(h, 0, C.byref(buf), C.byref(nb)) == 0
    assert nb.value == 4 * 240 * 320
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)
    env.sync()


def test_another_unit_replays_and_a_float_batch_follows(pool):
    own = pool.other("captures")
    n = 3
    k1 = [("Q1", 0), ("Q1", 1)]
    k2 = [("Qhalf", 0), ("Qhalf", 1)]
    # the yardsticks first: a context's first hpe_pipeline_begin allocates the single pipeline's
    # buffers, which starts a new graph epoch -- between the two batches it would hide the replay
    for k in k1 + k2:
        own.single(k, pool.f[k][:n], 1)
    a = check_lanes(pool, own, k1, n, 1, tag="units")
    c1 = own.ctx.graph_captures()
    b = check_lanes(pool, own, k2, n, 1, tag="units")
    assert own.ctx.graph_captures() == c1  # the unit is device memory, not part of any graph
    assert not np.array_equal(a, b)  # another quantisation, another trajectory
    # a float batch on the same context, the same state buffer and pinned buffers
    got = own.live([pool.f[k][:n] for k in k2], 1, "f32", tag="units")
    assert own.ctx.graph_captures() > c1  # the format is part of the key
    for lane, k in enumerate(k2):
        want = own.single(k, pool.f[k][:n], 1)
        for f in range(n):
            assert np.array_equal(got[f, lane], want[f]), (lane, f)
    assert np.array_equal(got, b)
