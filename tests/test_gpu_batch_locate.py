"""hpe_batch_pipeline_locate and hpe_batch_locate_result: the hand of a live batch's lanes found in
their current raw frames on the device -- window, re-prepared frame and placed row.

The yardstick is existing code: a live batch begun with whole-frame windows, located, then
tracked equals, bit for bit, a second batch begun with init[b] = the located windows and x0 = the
located rows -- and those windows and rows are the numpy mirror's (hpe/locate.py on the lane's raw
frame, hpe_build_spheres for the template's centres), never the call's own output.

Shapes: P = 32 and 4 generations (maxiter 5); the kernels under test do not depend on P.  16
lanes with a scene each (hpe.synth.rig_scene around a rendered hand: wall, forearm, speckle), the
empty frame at lanes 0 and 15; 3 frames per lane.  One tracking context for the whole file.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF, NL = 32, 5, 3, 16
FOCAL = 241.42
UNIT = 0.25        # mm per count of the u16 frames
MXY, MZ = 2.0, 3.0  # the FOLLOW windows' margins


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Env:
    def __init__(self):
        import hpe
        import torch
        from hpe import _lib, locate, synth, window
        self.hpe, self.torch, self._lib, self.locate, self.window = hpe, torch, _lib, locate, window
        self.hand = hpe.reference_hand(device=0)
        self.ctx = self.hand.ctx
        self.lib = self.ctx.lib
        ub, lb, sd = hpe.reference_bounds()
        self.pso = hpe.PSO()
        self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        self.pso._push(self.ctx)
        x0 = np.asarray(hpe.X0, dtype=np.float64)
        # lane b's stream: a trajectory of its own, moved sideways, in front of the rig's clutter
        self.f32, self.u16 = [], []
        for b in range(NL):
            if b in (0, NL - 1):
                fr = [np.zeros((240, 320), np.float32)] * NF
            else:
                poses = synth.trajectory(NF, seed=b)
                poses[:, 3] += (b % 5 - 2) * 2.0
                poses[:, 4] += (b % 3 - 1) * 1.5
                fr = [synth.rig_scene(self.ctx.render_depth(th), th[3:6], FOCAL, seed=b) for th in poses]
            self.f32.append(fr)
            self.u16.append([np.round(f / np.float32(UNIT)).astype(np.uint16) for f in fr])
        # the lanes' templates (the caller's guess of rotation and digits) and start rows
        self.T = np.stack([x0] * NL)
        self.T[:, 0] += np.arange(NL)
        self.T[:, 7] += 0.5 * np.arange(NL)
        self.start = np.zeros((NL, 27))
        self.start[:, :26] = x0
        self.start[:, 3] += 0.25 * np.arange(NL)
        self.st = torch.zeros((NL, 27), dtype=torch.float64, device="cuda:0")
        self._hands = {}
        self._mirror = {}
        self.sync()

    def close(self):
        for h in self._hands.values():
            h.ctx.close()
        self.ctx.close()

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def err(self):
        return self.lib.hpe_last_error(self.ctx.h)

    def frames(self, inp, lanes, f):
        src = self.u16 if inp == "u16" else self.f32
        return [src[b][f].copy() for b in lanes]

    def mirror(self, inp, b, f=0, params=None):
        """The numpy mirror's result on frame f of lane b (computed once, shared, never changed)."""
        key = (inp, b, f, params)
        if key not in self._mirror:
            p = self.locate.DEFAULTS if params is None else params
            self._mirror[key] = (self.locate.locate(self.u16[b][f], FOCAL, p, unit_mm=UNIT)
                                 if inp == "u16" else self.locate.locate(self.f32[b][f], FOCAL, p))
        return self._mirror[key]

    def hand_ctx(self, scales):
        if scales not in self._hands:
            self._hands[scales] = self.hpe.scaled_hand(*scales)
        return self._hands[scales]

    def placed(self, res, template, row, hand=None):
        """The row the placement rule gives lane's `row` (a not-found lane's stays as it is)."""
        if not res.found:
            return row.copy()
        S = (hand or self.hand).build_batch(template)[0][0]
        out = row.copy()
        out[:26] = self.locate.place(self.locate.camera_centres(S), template, res.centre)
        return out

    def expected(self, inp, lanes, f=0):
        """The mirror's windows (a not-found lane keeps the whole frame) and rows of `lanes`."""
        res = [self.mirror(inp, b, f) for b in lanes]
        wins = [r.window if r.found else self.window.WHOLE for r in res]
        rows = np.stack([self.placed(r, self.T[b], self.start[b]) for r, b in zip(res, lanes)])
        return res, wins, rows

    def states(self, B):
        return self.st[:B]

    def put(self, st, rows):
        st.copy_(self.torch.from_numpy(np.ascontiguousarray(rows)))
        self.torch.cuda.synchronize()

    def begin(self, inp, lanes, mode, init, rows, form="auto"):
        B = len(lanes)
        self.ctx.set_batch_form(form)
        self.ctx.set_batch_window(mode, init, MXY, MZ)
        st = self.states(B)
        self.put(st, rows)
        self.ctx.batch_pipeline_begin(self.frames(inp, lanes, 0), input=inp, unit_mm=UNIT)
        return st

    def track(self, inp, lanes, st, n, refine=1, first=0):
        """n tracked frames from frame `first`; the states after each (n x B x 27)."""
        out = []
        for f in range(first, first + n):
            nxt = self.frames(inp, lanes, f + 1) if f + 1 < first + n else None
            self.ctx.track_batch_pipelined(P, refine, st.data_ptr(), nxt)
            self.sync()
            out.append(st.cpu().numpy().copy())
        return np.array(out)

    def windows(self, B):
        return [self.ctx.batch_windows_readback(p, B) for p in (0, 1)]

    def end(self):
        """Leave the context as the next test expects it, whatever state a failure left."""
        try:
            if self.lib.hpe_batch_pending(self.ctx.h, C.byref(C.c_uint32())) == 0:
                self.ctx.track_batch_pipelined(P, 0, self.st.data_ptr(), None)
        except self.hpe.HpeError:
            pass
        self.sync()
        for fn in (lambda: self.ctx.set_batch_report(0), lambda: self.ctx.set_batch_hands(None),
                   lambda: self.ctx.set_batch_pacing("lockstep"), lambda: self.ctx.set_batch_form("auto"),
                   lambda: self.ctx.set_batch_window("off")):
            fn()


@pytest.fixture(scope="module")
def env_module():
    e = Env()
    yield e
    e.close()


@pytest.fixture
def env(env_module):
    yield env_module
    env_module.end()


def same_result(got, want):
    assert np.array_equal([got.found, got.k_near, got.m1, got.m2],
                          [want.found, want.k_near, want.m1, want.m2]), (got, want)
    assert np.array_equal(bits(got.px), bits(want.px)) and np.array_equal(bits(got.centre), bits(want.centre))
    assert np.array_equal(got.window[:4], want.window[:4])
    assert np.array_equal(bits(got.window[4:]), bits(want.window[4:]))


@pytest.mark.parametrize("form", ["auto", "wave"])
@pytest.mark.parametrize("inp", ["f32", "u16"])
@pytest.mark.parametrize("mode", ["follow", "fixed"])
def test_yardstick_sixteen_lanes(env, mode, inp, form):
    lanes = list(range(NL))
    res, wins, rows = env.expected(inp, lanes)
    assert [r.found for r in res] == [0] + [1] * (NL - 2) + [0]  # the empty scenes at both ends
    whole = [env.window.WHOLE] * NL
    # batch A: whole-frame windows, then the locate
    st = env.begin(inp, lanes, mode, whole, env.start, form)
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T)
    env.sync()
    got_rows = st.cpu().numpy()
    w0, w1 = env.windows(NL)
    assert np.array_equal(bits(got_rows), bits(rows))
    assert w0 == wins                                   # the current parity
    assert w1 == (wins if mode == "fixed" else whole)   # the other one: FIXED alone
    for b in lanes:
        seq, r = env.ctx.batch_locate_result(b)
        assert seq == 1
        same_result(r, res[b])
    a = env.track(inp, lanes, st, NF)
    # batch B: begun with the located windows and rows
    st = env.begin(inp, lanes, mode, wins, rows, form)
    b_ = env.track(inp, lanes, st, NF)
    assert np.array_equal(bits(a), bits(b_))
    # the premise: the locate mattered -- a located lane's window and row are not the begin's
    assert wins[1] != env.window.WHOLE and not np.array_equal(rows[1, 3:6], env.start[1, 3:6])


def test_subset_mask_leaves_the_other_lanes_alone(env):
    lanes, sel = [1, 2, 3, 4], 0b0110
    whole = [env.window.WHOLE] * 4
    st = env.begin("f32", lanes, "follow", whole, env.start[lanes])
    plain = env.track("f32", lanes, st, NF)
    st = env.begin("f32", lanes, "follow", whole, env.start[lanes])
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes], lanes=sel)
    env.sync()
    rows = st.cpu().numpy()
    w = env.windows(4)
    _, wins, want = env.expected("f32", lanes)
    for k in range(4):
        if sel >> k & 1:
            assert np.array_equal(bits(rows[k]), bits(want[k])) and w[0][k] == wins[k]
        else:
            assert np.array_equal(bits(rows[k]), bits(env.start[lanes[k]]))
            assert w[0][k] == env.window.WHOLE
        assert w[1][k] == env.window.WHOLE
    assert env.ctx.batch_locate_result(0)[0] == 0 and env.ctx.batch_locate_result(1)[0] == 1
    got = env.track("f32", lanes, st, NF)
    for k in range(4):
        if sel >> k & 1:
            assert not np.array_equal(bits(got[:, k]), bits(plain[:, k]))
        else:
            assert np.array_equal(bits(got[:, k]), bits(plain[:, k]))


def test_lane_hands(env):
    """The placement under each lane's own hand: the same scene and template in three lanes."""
    scales = [None, (0.9, 0.85), (1.15, 1.1)]
    hands = [env.hand if s is None else env.hand_ctx(s) for s in scales]
    lanes = [5, 5, 5]
    env.ctx.set_batch_hands(hands)
    st = env.begin("f32", lanes, "fixed", [env.window.WHOLE] * 3, env.start[lanes])
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[5])
    env.sync()
    rows = st.cpu().numpy()
    res = env.mirror("f32", 5)
    for k, h in enumerate(hands):
        S = env.locate.camera_centres(h.build_batch(rows[k, :26])[0][0])
        off = env.locate.centroid(S) - np.array(res.centre)
        print("lane", k, "centroid - centre", off)
        assert np.abs(off).max() <= 1e-9
        assert np.array_equal(bits(rows[k]), bits(env.placed(res, env.T[5], env.start[5], h)))
    assert not np.array_equal(rows[0, 3:6], rows[1, 3:6])  # the hand matters
    assert not np.array_equal(rows[0, 3:6], rows[2, 3:6])
    env.track("f32", lanes, st, 1)


def test_free_pacing_late_joiner(env):
    lanes = [1, 2, 3]
    env.ctx.set_batch_pacing("free")
    env.ctx.set_batch_form("auto")
    env.ctx.set_batch_window("follow", [env.window.WHOLE] * 3, MXY, MZ)
    st = env.states(3)
    env.put(st, env.start[lanes])
    fr = env.frames("f32", lanes, 0)
    env.ctx.batch_pipeline_begin([fr[0], None, fr[2]])
    assert env.ctx.batch_pending() == 0b101
    before = (st.cpu().numpy(), env.windows(3))
    for sel in (0b010, 0b111):  # lane 1 holds no prepared frame
        with pytest.raises(env.hpe.HpeError, match="hpe error -3"):
            env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes], lanes=sel)
        assert b"hold no prepared frame" in env.err()
    env.sync()
    assert np.array_equal(bits(st.cpu().numpy()), bits(before[0])) and env.windows(3) == before[1]
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes])  # None: the pending lanes
    # lane 1 joins: given its first frame in a call, located and optimised before the next
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [None, fr[1], None])
    assert env.ctx.batch_pending() == 0b010
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes], lanes=0b010)
    env.sync()
    rows = st.cpu().numpy()
    _, wins, want = env.expected("f32", lanes)
    assert np.array_equal(bits(rows[1]), bits(want[1]))
    assert env.ctx.batch_windows_readback(1, 3)[1] == wins[1]  # its frame went into parity 1
    assert [env.ctx.batch_locate_result(b)[0] for b in range(3)] == [1, 1, 1]
    env.ctx.batch_pipeline_optimise(P, st.data_ptr(), lanes=0b010)
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)
    env.sync()
    out = st.cpu().numpy()
    assert np.isfinite(out[1]).all() and not np.array_equal(out[1], rows[1])
    assert np.array_equal(bits(out[[0, 2]]), bits(rows[[0, 2]]))  # idle in that call


def test_recovery_of_a_lost_lane(env):
    """A lane whose row is overwritten with a far-off pose follows its window off the image and is
    reported LOST; locate + hpe_batch_pipeline_optimise on its current frame bring it back: the
    next TRACK report is healthy."""
    _lib = env._lib
    lanes = [6, 7]
    frames = [env.f32[b][0] for b in lanes]  # a still scene per lane
    env.ctx.set_batch_report(4, (np.inf, 1000, 1))
    st = env.begin("f32", lanes, "follow", [env.window.WHOLE] * 2, env.start[lanes])
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes])
    env.ctx.batch_pipeline_optimise(P, st.data_ptr())

    def step():
        env.ctx.track_batch_pipelined(P, 0, st.data_ptr(), [f.copy() for f in frames])
        env.sync()
        return [env.ctx.batch_report(b) for b in range(2)]

    r = step()
    assert [x.kind for x in r] == [_lib.REPORT_TRACK] * 2 and [x.flags for x in r] == [0, 0]
    rows = st.cpu().numpy()
    rows[0, 3] += 70.0  # 70 cm to the side: the pose rule's window leaves the image
    env.put(st, rows)
    flags = []
    for _ in range(2):
        r = step()
        flags.append(r[0].flags)
        assert r[1].flags == 0
    print("lane 0 flags after the overwrite", flags, "n", r[0].n)
    assert flags[1] & _lib.REPORT_F_LOST and env.ctx.batch_lost() == 0b01
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes], lanes=0b01)
    env.ctx.batch_pipeline_optimise(P, st.data_ptr(), lanes=0b01)
    r = step()
    assert r[0].kind == _lib.REPORT_TRACK and r[0].flags == 0 and r[1].flags == 0
    assert r[0].n >= 1000 and env.ctx.batch_lost() == 0
    assert env.ctx.batch_locate_result(0)[0] == 2 and env.ctx.batch_locate_result(1)[0] == 1


def test_no_graph_is_captured(env):
    torch = env.torch
    lanes = [1, 2]
    whole = [env.window.WHOLE] * 2
    counts = []
    keep = []
    for with_locate in (False, True):
        st = torch.zeros((2, 27), dtype=torch.float64, device="cuda:0")  # a graph key of its own
        keep.append(st)
        env.ctx.set_batch_window("follow", whole, MXY, MZ)
        env.put(st, env.start[lanes])
        c0 = env.ctx.graph_captures()
        env.ctx.batch_pipeline_begin(env.frames("f32", lanes, 0))
        for f in range(NF):
            if with_locate:
                for _ in range(2 if f == 1 else 1):  # between two track calls, and a second one
                    c = env.ctx.graph_captures()
                    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes])
                    assert env.ctx.graph_captures() == c
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(),
                                          env.frames("f32", lanes, f + 1) if f + 1 < NF else None)
        env.sync()
        counts.append(env.ctx.graph_captures() - c0)
    print("graphs captured without / with the locates", counts)
    assert counts[0] == counts[1] and counts[0] >= 1


def test_result_without_synchronisation(env):
    """Nothing synchronises between the begin and the waits: the wait alone delivers the result,
    which is the mirror's; seq counts each lane's locates since the begin."""
    lanes = [3, 0, 9]
    st = env.begin("u16", lanes, "fixed", [env.window.WHOLE] * 3, env.start[lanes])
    assert [env.ctx.batch_locate_result(b)[0] for b in range(3)] == [0, 0, 0]  # none yet
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes])
    first = [env.ctx.batch_locate_result(b, 5000, raw=True) for b in range(3)]
    env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes], lanes=0b110)
    second = [env.ctx.batch_locate_result(b, 5000, raw=True) for b in range(3)]
    assert [(r.seq, r.lane) for r in first] == [(1, 0), (1, 1), (1, 2)]
    assert [(r.seq, r.lane) for r in second] == [(1, 0), (2, 1), (2, 2)]
    res, wins, rows = env.expected("u16", lanes)
    for r, want in zip(first + second, res + res):
        same_result(env.ctx._locate_result(r, False), want)
    assert [r.found for r in res] == [1, 0, 1]
    env.sync()
    assert np.array_equal(bits(st.cpu().numpy()), bits(rows))
    # a new begin starts the count again
    env.track("u16", lanes, st, 1)
    env.begin("u16", lanes, "fixed", [env.window.WHOLE] * 3, env.start[lanes])
    assert [env.ctx.batch_locate_result(b)[0] for b in range(3)] == [0, 0, 0]


def test_refusals_change_nothing(env):
    _lib, locate = env._lib, env.locate
    lib, h = env.lib, env.ctx.h
    lanes = [1, 2]
    T = np.ascontiguousarray(env.T[lanes])
    tp = T.ctypes.data_as(C.POINTER(C.c_double))
    out = _lib.Locate()

    def call(B=2, states=None, mask=0b11, tmpl=tp, **kw):
        arr = None
        if kw:
            arr = (_lib.LocateParams * 2)(env.ctx._locate_params(locate.DEFAULTS),
                                          env.ctx._locate_params(locate.DEFAULTS._replace(**kw)))
        return lib.hpe_batch_pipeline_locate(h, B, C.c_void_p(states), mask, tmpl, arr)

    st = env.states(2)
    # no live batch (none begun in this test; the fixture ended the last one)
    env.ctx.set_batch_window("follow", [env.window.WHOLE] * 2, MXY, MZ)
    env.put(st, env.start[lanes])
    assert call(states=st.data_ptr()) == _lib.HPE_E_STATE and b"no live batch" in env.err()
    st = env.begin("f32", lanes, "follow", [env.window.WHOLE] * 2, env.start[lanes])
    sp = st.data_ptr()
    before = (st.cpu().numpy(), env.windows(2))
    assert call(states=None) == _lib.HPE_E_ARG
    assert call(states=sp, tmpl=None) == _lib.HPE_E_ARG
    for kw in (dict(bin=0.0), dict(bin=-0.5), dict(bin=np.nan), dict(slab=-1.0), dict(slab=np.inf),
               dict(half_xy=-1.0), dict(half_z=np.nan), dict(skip=-1), dict(min_pixels=-3)):
        assert call(states=sp, **kw) == _lib.HPE_E_ARG, kw
    assert call(states=sp, mask=0) == _lib.HPE_E_ARG
    assert call(states=sp, mask=0b100) == _lib.HPE_E_ARG
    assert call(B=0, states=sp) == _lib.HPE_E_ARG and call(B=17, states=sp) == _lib.HPE_E_ARG
    assert call(B=3, states=sp, mask=0b001) == _lib.HPE_E_STATE and b"began with 2" in env.err()
    assert lib.hpe_batch_locate_result(h, 2, 0, C.byref(out)) == _lib.HPE_E_ARG
    assert lib.hpe_batch_locate_result(h, -1, 0, C.byref(out)) == _lib.HPE_E_ARG
    assert lib.hpe_batch_locate_result(h, 0, 0, None) == _lib.HPE_E_ARG
    env.sync()
    assert np.array_equal(bits(st.cpu().numpy()), bits(before[0])) and env.windows(2) == before[1]
    assert env.ctx.batch_locate_result(0)[0] == 0  # nothing was enqueued
    assert call(states=sp) == 0  # ... and the call that follows works
    assert call(states=sp, mask=0b01, bin=-1.0) == 0  # an unselected lane's entry is not read
    env.sync()
    assert np.array_equal(bits(st.cpu().numpy()), bits(env.expected("f32", lanes)[2]))
    env.track("f32", lanes, st, 1)
    # window mode OFF: the table is not read
    env.ctx.set_batch_window("off")
    env.put(st, env.start[lanes])
    env.ctx.batch_pipeline_begin(env.frames("f32", lanes, 0))
    assert call(states=sp) == _lib.HPE_E_STATE and b"windows are off" in env.err()
    env.sync()
    assert np.array_equal(bits(st.cpu().numpy()), bits(env.start[lanes]))
    env.track("f32", lanes, st, 1)
    assert call(states=sp) == _lib.HPE_E_STATE and b"no live batch" in env.err()  # the batch ended


@pytest.mark.parametrize("in_place", [False, True])
def test_host_runs_ahead_of_the_locate(env, in_place):
    """The locate kernels read the lanes' pinned buffers in place, behind whatever the stream still
    holds.  A host that never synchronises enqueues the locate, the track call of those frames and
    the track call after it, whose frames go into the same pinned buffers (copied, or filled in
    place through hpe_batch_frame_buffer): the buffers must stay intact until the locate has read
    them.  The run equals the one that synchronises after every call; the frames that refill the
    buffers are other scenes, so a locate that read a refilled buffer cannot pass."""
    lanes, other = [1, 2, 3], [9, 10, 11]
    whole = [env.window.WHOLE] * 3
    res, wins, rows = env.expected("f32", lanes)

    def run(sync):
        wait = env.sync if sync else (lambda: None)
        st = env.begin("f32", lanes, "follow", whole, env.start[lanes])
        for _ in range(8):  # work ahead of the locate on the stream: the host gets far ahead of it
            env.ctx.batch_pipeline_optimise(P, st.data_ptr())
        wait()
        env.ctx.batch_pipeline_locate(st.data_ptr(), env.T[lanes])
        wait()
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), env.frames("f32", lanes, 1))
        wait()
        nxt = env.frames("f32", other, 0)  # into the buffers the locate reads
        if in_place:
            for b in range(3):
                buf = env.ctx.batch_frame_buffer(b)
                buf[:] = nxt[b]
                nxt[b] = buf
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), nxt)
        wait()
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)
        env.sync()
        return st.cpu().numpy(), [env.ctx.batch_locate_result(b)[1] for b in range(3)], env.windows(3)

    want = run(True)   # (it also captures the graphs: the second run's host only replays)
    got = run(False)
    for r, m in zip(got[1], res):
        same_result(r, m)
    assert got[2] == want[2]
    assert np.array_equal(bits(got[0]), bits(want[0]))
