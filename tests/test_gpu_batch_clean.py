"""Lane cleaning of the live batch (hpe_set_batch_clean): every lane's 16-bit frame cleaned on the
device by k_clean_b, ahead of the preparation, with the lane's own parameters.

The yardstick is always the single pipelined loop (hpe_pipeline_begin + hpe_track_pipelined) of
one stream alone on hpe.depth_u16_to_mm(hpe.clean.clean(view.reduce(frame))) -- the numpy mirrors
of the view and of the cleaning rule -- compared with np.array_equal on the 27-double state after
EVERY frame; never a batch, never the kernel.

Streams are hpe.synth.camera_noise over the quantised renders of tests/test_gpu_batch_input.py:
flying pixels on the silhouette and speckle around the hand.  The inputs are asserted: on every
frame of every lane cleaning changes pixels, inside the lane's window where there is one, and the
hand lies in front of the noise's background.  View lanes embed the noisy frame in a poisoned
camera frame as tests/test_gpu_batch_view.py does.

Small shapes: P = 64, maxiter 7, at most 4 frames per lane and 3 lanes, but for one 16-lane case
of 2 frames.  One context runs every batch but the capture counts, the wave forms and the lane
hands, which need contexts of their own.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_batch_input import FOCAL, MXY, MZ, P, Env, follow_yard, quantise
from test_gpu_batch_view import embed

pytestmark = pytest.mark.gpu

NF = 4
UNITS = {"Q1": np.float32(1.0), "Qhalf": np.float32(0.5)}
BACKGROUND_MM = 800


class Pool:
    """The module's context, noisy streams, views and parameters; frames and yardsticks are
    built once, shared and never changed."""

    def __init__(self):
        from hpe import clean, synth
        from hpe.view import View
        self.clean = clean
        self.env = Env()
        e = self.env
        self.render = {s: [np.ascontiguousarray(e.ctx.render_depth(th), dtype=np.float32)
                           for th in synth.trajectory(NF, s)] for s in range(3)}
        self.noisy = {}
        for u, unit in UNITS.items():
            for s in range(3):
                qs = [quantise(r, unit) for r in self.render[s]]
                bg = int(BACKGROUND_MM / unit)
                for q in qs:  # the hand lies in front of the background
                    assert q.any() and q.max() + 60 / unit < bg
                self.noisy[(u, s)] = [synth.camera_noise(q, 100 * s + k, background=bg,
                                                         jitter=int(30 / unit))
                                      for k, q in enumerate(qs)]
                assert all(not np.array_equal(a, q) for a, q in zip(self.noisy[(u, s)], qs))
        self.views = {
            None: None,
            "640x480 step 2": View(640, 480, 640, 0, 0, 2),
            "848x480 step 2 pitch 896": View(848, 480, 896, 0, 104, 2),
            "1024x1024 step 3 odd origin": View(1024, 1024, 1024, 151, 31, 3),
            "flip": View(640, 480, 672, 0, 0, 2, 1),
        }
        self.par = {"default": clean.defaults(1.0), "loose": clean.Clean(25, 2, 0),
                    "strict": clean.Clean(8, 4, clean.MEDIAN), "default half": clean.defaults(0.5)}
        self.cam, self.model = {}, {}
        self.cleaned, self.f = {}, {}
        self.others = {}

    def raw(self, vname, key):
        """(what the lane delivers, its 240x320 model frames): the noisy frames themselves, or
        camera frames that hold them under view vname."""
        k = (vname, key)
        if k not in self.cam:
            v = self.views[vname]
            if v is None:
                self.cam[k] = self.model[k] = self.noisy[key]
            else:
                self.cam[k] = [embed(v, q, seed) for seed, q in enumerate(self.noisy[key])]
                self.model[k] = [v.reduce(c) for c in self.cam[k]]
                want = [q[:, ::-1] if v.flip else q for q in self.noisy[key]]
                assert all(np.array_equal(m, w) for m, w in zip(self.model[k], want))
        return self.cam[k], self.model[k]

    def frames(self, vname, key, pname):
        """(the mirror's cleaned uint16 frames, their float conversion) of a lane."""
        k = (vname, key, pname)
        if k not in self.f:
            model = self.raw(vname, key)[1]
            self.cleaned[k] = [self.par[pname].apply(m) for m in model]
            for m, c in zip(model, self.cleaned[k]):  # cleaning changes every frame
                assert not np.array_equal(m, c) and c.any()
            self.f[k] = [self.env.hpe.depth_u16_to_mm(c, UNITS[key[0]]) for c in self.cleaned[k]]
        return self.cleaned[k], self.f[k]

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


def begin_kw(pool, lanes):
    """The begin's keywords for lanes = [(view name or None, stream key, parameter name)]: all
    plain u16 lanes or all view lanes."""
    unit = UNITS[lanes[0][1][0]]
    if lanes[0][0] is None:
        assert all(v is None for v, _, _ in lanes)
        return dict(input="u16", unit_mm=unit, focal=FOCAL)
    return dict(input="view", views=[pool.views[v] for v, _, _ in lanes], unit_mm=unit, focal=FOCAL)


def end_live(env, st):
    """A live batch still in progress (a check failed half way) is ended, so that the settings
    can be put back; then the stream is synchronised."""
    buf = C.c_void_p()
    if env.lib.hpe_batch_frame_buffer(env.ctx.h, 0, C.byref(buf), None) == 0:
        env.ctx.track_batch_pipelined(P, 0, st.data_ptr(), None)
    env.sync()


def live_clean(pool, env, lanes, refine=1, in_place=(), x0s=None, tag=None, n=NF, readback=False):
    """The cleaned batch over the lanes, a frame per lane and call: the states after every frame
    (n x B x 27).  readback: after every call the lanes' cleaned frames of both parities are read
    back and compared with the mirror's."""
    raws = [pool.raw(v, k)[0][:n] for v, k, _ in lanes]
    B = len(lanes)
    st = env.batch_states(B, tag)
    st.copy_(env.torch.from_numpy(np.stack([env.start(None if x0s is None else x0s[b])
                                            for b in range(B)])))
    env.torch.cuda.synchronize()
    out = []
    env.ctx.set_batch_clean([pool.par[p] for _, _, p in lanes])
    try:
        env.ctx.batch_pipeline_begin([r[0].copy() for r in raws], **begin_kw(pool, lanes))
        for f in range(n):
            nxt = None
            if f + 1 < n:
                nxt = []
                for b, r in enumerate(raws):
                    if b in in_place:
                        buf = env.ctx.batch_frame_buffer(b)
                        assert buf.dtype == np.uint16 and buf.shape == r[f + 1].shape
                        buf[:] = r[f + 1]
                        nxt.append(buf)
                    else:
                        nxt.append(r[f + 1].copy())
            env.ctx.track_batch_pipelined(P, refine, st.data_ptr(), nxt)
            env.sync()
            out.append(st.cpu().numpy().copy())
            if readback:
                for b, lane in enumerate(lanes):
                    want = pool.frames(*lane)[0]
                    assert np.array_equal(env.ctx.batch_clean_readback(f & 1, b), want[f]), (b, f)
                    if f + 1 < n:
                        assert np.array_equal(env.ctx.batch_clean_readback((f + 1) & 1, b), want[f + 1]), (b, f)
    finally:
        end_live(env, st)
        env.ctx.set_batch_clean(None)
    return np.array(out)


def check_clean_lanes(pool, env, lanes, refine=1, yard=None, n=NF, **kw):
    got = live_clean(pool, env, lanes, refine, n=n, **kw)
    for b, lane in enumerate(lanes):
        want = (yard or env).single(("clean",) + lane, pool.frames(*lane)[1][:n], refine)
        for f in range(n):
            assert np.array_equal(got[f, b], want[f]), (lane, b, f)
    return got


# ---- 1. plain u16 lanes and view lanes, parameters per lane
PLAIN = [(None, ("Q1", 0), "default"), (None, ("Q1", 1), "loose"), (None, ("Q1", 2), "strict")]
VIEWED = [("848x480 step 2 pitch 896", ("Q1", 0), "strict"), ("flip", ("Q1", 1), "default"),
          ("1024x1024 step 3 odd origin", ("Q1", 2), "loose")]


@pytest.mark.parametrize("refine", [1, 0])
def test_plain_lanes_with_distinct_parameters(pool, env, refine):
    got = check_clean_lanes(pool, env, PLAIN, refine, readback=refine == 1)
    assert np.isfinite(got).all()
    # cleaning matters: the raw noisy stream tracks to other states
    noisy_f = [env.hpe.depth_u16_to_mm(q, 1.0) for q in pool.noisy[("Q1", 0)]]
    assert not np.array_equal(got[:, 0], env.single(("noisy", 0), noisy_f, refine))


def test_view_lanes_with_distinct_parameters(pool, env):
    got = check_clean_lanes(pool, env, VIEWED, readback=True)
    assert np.isfinite(got).all()
    assert env.ctx.batch_views_readback(3) == [pool.views[v] for v, _, _ in VIEWED]


@pytest.mark.parametrize("order", [(1, 2, 0), (2, 0, 1)])
def test_the_same_parameters_permuted_across_lanes(pool, env, order):
    names = [PLAIN[k][2] for k in order]
    lanes = [(v, k, names[b]) for b, (v, k, _) in enumerate(PLAIN)]
    got = check_clean_lanes(pool, env, lanes)
    base = check_clean_lanes(pool, env, PLAIN)
    for b in range(3):  # each lane took its own entry: another parameter set, other states
        assert not np.array_equal(got[:, b], base[:, b]), b


def test_a_fractional_unit(pool, env):
    check_clean_lanes(pool, env, [(None, ("Qhalf", 0), "default half"),
                                  (None, ("Qhalf", 1), "strict")], n=3)
    check_clean_lanes(pool, env, [("640x480 step 2", ("Qhalf", 2), "default half")], n=3)


def test_sixteen_lanes(pool, env):
    names = ["default", "loose", "strict"]
    lanes = [("flip", ("Q1", 0), "strict")] + \
            [("640x480 step 2", ("Q1", b % 3), names[b % 3]) for b in range(1, 15)] + \
            [("1024x1024 step 3 odd origin", ("Q1", 1), "loose")]
    got = check_clean_lanes(pool, env, lanes, n=2, tag="sixteen", readback=True)
    assert not np.array_equal(got[:, 0], got[:, 15])
    plain = [(None, ("Q1", b % 3), names[(b + 1) % 3]) for b in range(16)]
    check_clean_lanes(pool, env, plain, n=2, tag="sixteen")


def test_in_place_delivery(pool, env):
    for lanes in (PLAIN, VIEWED):
        for in_place in ({0, 1, 2}, {1}):
            check_clean_lanes(pool, env, lanes, in_place=in_place, n=3)
    # hpe_batch_frame_buffer keeps its contract: the lane's own frame size, distinct buffers
    raws = [pool.raw(v, k)[0] for v, k, _ in VIEWED]
    st = env.batch_states(3)
    env.ctx.set_batch_clean([pool.par[p] for _, _, p in VIEWED])
    try:
        env.ctx.batch_pipeline_begin([r[0] for r in raws], **begin_kw(pool, VIEWED))
        addr = []
        for b, (v, _, _) in enumerate(VIEWED):
            buf, nb = C.c_void_p(), C.c_size_t(0)
            assert env.lib.hpe_batch_frame_buffer(env.ctx.h, b, C.byref(buf), C.byref(nb)) == 0
            assert nb.value == 2 * pool.views[v].pitch * pool.views[v].height
            addr.append(buf.value)
        assert len(set(addr)) == 3
        env.ctx.track_batch_pipelined(P, 0, st.data_ptr(), None)
        env.sync()
    finally:
        end_live(env, st)
        env.ctx.set_batch_clean(None)


# ---- 2. windows with lane hands
SCALES = [(0.9, 0.85), (1.1, 1.2)]


def hand_yards(pool):
    return [pool.other(("hand", s), hand=s) for s in SCALES]


def test_fixed_windows_with_lane_hands(pool, env):
    W = env.window
    lanes = [(None, ("Q1", 1), "default"), (None, ("Q1", 2), "strict")]
    yards = hand_yards(pool)
    w = env.rule(env.x0)
    half = W.Window(w.row_lo, w.row_hi, w.col_lo, (w.col_lo + w.col_hi) // 2, w.z_lo, w.z_hi)
    wins = [half, w]
    n = 3
    fs = [pool.frames(*lane)[1][:n] for lane in lanes]
    for b, (v, k, _) in enumerate(lanes):  # cleaning changes pixels inside the lane's window
        for f in range(n):
            noisy = env.hpe.depth_u16_to_mm(pool.raw(v, k)[1][f], 1.0)
            assert not np.array_equal(W.apply(noisy, wins[b]), W.apply(fs[b][f], wins[b])), (b, f)
    env.ctx.set_batch_window("fixed", wins, MXY, MZ)
    env.ctx.set_batch_hands([y.hand for y in yards])
    try:
        got = live_clean(pool, env, lanes, tag="hands", n=n)
    finally:
        env.ctx.set_batch_hands(None)
        env.ctx.set_batch_window("off")
    for b, lane in enumerate(lanes):
        want = yards[b].single(("clean fixed",) + lane + (tuple(wins[b]),),
                               [W.apply(f, wins[b]) for f in fs[b]], 1)
        for f in range(n):
            assert np.array_equal(got[f, b], want[f]), (b, f)


def test_follow_windows_with_lane_hands(pool, env):
    W = env.window
    lanes = [("1024x1024 step 3 odd origin", ("Q1", 0), "default"), ("flip", ("Q1", 1), "loose")]
    yards = hand_yards(pool)
    fs = [pool.frames(*lane)[1] for lane in lanes]
    x0s = [env.x0, env.x0]
    inits = [yards[b].rule(x0s[b]) for b in range(2)]
    follow = [follow_yard(yards[b], fs[b], x0s[b], inits[b]) for b in range(2)]
    for b, (v, k, _) in enumerate(lanes):  # inside the windows the yardstick followed, too
        wins = [inits[b], yards[b].rule(x0s[b])] + [yards[b].rule(s) for s in follow[b][1][:NF - 2]]
        for f in range(NF):
            noisy = env.hpe.depth_u16_to_mm(pool.raw(v, k)[1][f], 1.0)
            assert np.array_equal(W.apply(fs[b][f], wins[f]), follow[b][0][f])
            assert not np.array_equal(W.apply(noisy, wins[f]), follow[b][0][f]), (b, f)
    env.ctx.set_batch_window("follow", inits, MXY, MZ)
    env.ctx.set_batch_hands([y.hand for y in yards])
    try:
        got = live_clean(pool, env, lanes, x0s=x0s, tag="hands")
    finally:
        env.ctx.set_batch_hands(None)
        env.ctx.set_batch_window("off")
    for b in range(2):
        for f in range(NF):
            assert np.array_equal(got[f, b], follow[b][1][f]), (b, f)


# ---- 3. pacing, forms, reports, optimise
@pytest.mark.parametrize("lanes", [PLAIN, VIEWED], ids=["u16", "view"])
def test_free_pacing_with_a_gap_and_a_late_joiner(pool, env, lanes):
    torch = env.torch
    raws = [pool.raw(v, k)[0] for v, k, _ in lanes]
    sched = [{0, 1}, {0, 2}, {0, 1, 2}, {0, 1, 2}, None]  # lane 2 joins late, lane 1 skips a call
    st = env.batch_states(3, "paced")
    st.copy_(torch.from_numpy(np.stack([env.start(), env.start(), np.full(27, np.nan)])))
    torch.cuda.synchronize()
    took, tracked = [0, 0, 0], [[], [], []]

    def frames(step):
        if step is None:
            return None
        fr = [None] * 3
        for b in step:
            fr[b] = raws[b][took[b]].copy()
            took[b] += 1
        return fr

    # a lockstep batch first, so that lane 2's staging frame of parity 0 holds its frame 1 cleaned
    held = pool.frames(*lanes[2])[0]
    assert not np.array_equal(held[1], held[0])
    env.ctx.set_batch_clean([pool.par[p] for _, _, p in lanes])
    try:
        env.ctx.batch_pipeline_begin([r[1].copy() for r in raws], **begin_kw(pool, lanes))
        env.ctx.track_batch_pipelined(P, 0, st.data_ptr(), None)
        env.sync()
        st.copy_(torch.from_numpy(np.stack([env.start(), env.start(), np.full(27, np.nan)])))
        torch.cuda.synchronize()
        env.ctx.set_batch_pacing("free")
        env.ctx.batch_pipeline_begin(frames(sched[0]), **begin_kw(pool, lanes))
        # a lane without a frame has none cleaned: its workgroups left the staging frame alone
        assert np.array_equal(env.ctx.batch_clean_readback(0, 2), held[1])
        assert np.array_equal(env.ctx.batch_clean_readback(0, 0), pool.frames(*lanes[0])[0][0])
        for k in range(len(sched) - 1):
            pending = sched[k]
            if k == 1:
                st[2].copy_(torch.from_numpy(env.start()))
                torch.cuda.synchronize()
            prev = st.cpu().numpy().copy()
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), frames(sched[k + 1]))
            env.sync()
            now = st.cpu().numpy().copy()
            for b in range(3):
                if b in pending:
                    tracked[b].append(now[b])
                else:
                    assert np.array_equal(now[b].view(np.uint64), prev[b].view(np.uint64)), (b, k)
    finally:
        end_live(env, st)
        env.ctx.set_batch_clean(None)
        env.ctx.set_batch_pacing("lockstep")
    assert [len(t) for t in tracked] == [4, 3, 3] == took
    for b, lane in enumerate(lanes):
        want = env.single(("clean",) + lane, pool.frames(*lane)[1][:took[b]], 1)
        for f in range(took[b]):
            assert np.array_equal(tracked[b][f], want[f]), (b, f)


@pytest.mark.parametrize("wpp", [1, 2])
def test_wave_form(pool, wpp):
    lanes = [(None, ("Q1", 1), "default"), (None, ("Q1", 2), "loose")]
    own = pool.other(("wpp", wpp), wpp=wpp)  # a batch context that only forces the waves per particle
    assert own.ctx.batch_wave_wpp(P, 2) == wpp
    yard = pool.other(("wave", wpp), form="wave", wpp=wpp)
    own.ctx.set_batch_form("wave")
    try:
        got = check_clean_lanes(pool, own, lanes, yard=yard, n=3)
        check_clean_lanes(pool, own, VIEWED[:2], yard=yard, n=3)
    finally:
        own.ctx.set_batch_form("auto")
    assert np.isfinite(got).all()


def test_reports_equal_the_batch_on_mirror_cleaned_frames(pool, env):
    lanes = VIEWED[:2]
    n = 3

    def run(device):
        st = env.batch_states(2, "report")
        st.copy_(env.torch.from_numpy(np.stack([env.start(), env.start()])))
        env.torch.cuda.synchronize()
        src = [pool.raw(v, k)[0] if device else pool.frames(v, k, p)[0] for v, k, p in lanes]
        kw = begin_kw(pool, lanes) if device else dict(input="u16", unit_mm=1.0, focal=FOCAL)
        reps = []
        env.ctx.set_batch_report(4)
        env.ctx.set_batch_clean([pool.par[p] for _, _, p in lanes] if device else None)
        try:
            env.ctx.batch_pipeline_begin([s[0] for s in src], **kw)
            for f in range(n):
                env.ctx.track_batch_pipelined(P, 1, st.data_ptr(),
                                              [s[f + 1] for s in src] if f + 1 < n else None)
                env.sync()
                reps.append([env.ctx.batch_report(b, raw=True) for b in range(2)])
        finally:
            end_live(env, st)
            env.ctx.set_batch_clean(None)
            env.ctx.set_batch_report(0)
        return reps

    a, b_ = run(True), run(False)
    for f in range(n):
        for lane in range(2):
            x, y = a[f][lane], b_[f][lane]
            assert (x.seq, x.kind, x.n, x.flags) == (y.seq, y.kind, y.n, y.flags) and x.seq == f + 1
            for field in ("state", "joints", "px"):
                assert np.array_equal(np.array(getattr(x, field)), np.array(getattr(y, field))), (f, lane, field)
            want = env.single(("clean",) + lanes[lane], pool.frames(*lanes[lane])[1][:n], 1)[f]
            assert np.array_equal(np.array(x.state), want)


def test_batch_pipeline_optimise(pool, env):
    lanes = [(None, ("Q1", 1), "strict"), (None, ("Q1", 0), "default")]
    n, G = 2, 6
    yards = []
    for b, lane in enumerate(lanes):  # the single call on the cleaned frame, then the single loop
        f = pool.frames(*lane)[1]
        env.ctx.prepare_frame(8 + b, f[0])
        env.ctx.select_frame(8 + b)
        x = np.ascontiguousarray(env.x0, dtype=np.float64)
        out, bc, tr = np.zeros(27), C.c_double(0), np.zeros(G)
        env.ctx.check(env.lib.hpe_pso_optimise(env.ctx.h, env._lib.ptr(x, C.c_double), P,
                                               env._lib.ptr(out, C.c_double), C.byref(bc),
                                               env._lib.ptr(tr, C.c_double), G))
        out[26] = bc.value
        env.st1.copy_(env.torch.from_numpy(out))
        env.torch.cuda.synchronize()
        states = []
        env.ctx.pipeline_begin(f[0])
        for g in range(n):
            env.ctx.track_pipelined(P, 1, env.st1.data_ptr(), f[g + 1] if g + 1 < n else None)
            env.sync()
            states.append(env.st1.cpu().numpy().copy())
        yards.append((out, states))
    st = env.batch_states(2, "opt")
    st.copy_(env.torch.from_numpy(np.stack([env.start(), env.start()])))
    env.torch.cuda.synchronize()
    raws = [pool.raw(v, k)[0] for v, k, _ in lanes]
    env.ctx.set_batch_clean([pool.par[p] for _, _, p in lanes])
    try:
        env.ctx.batch_pipeline_begin([r[0] for r in raws], **begin_kw(pool, lanes))
        env.ctx.batch_pipeline_optimise(P, st.data_ptr())
        env.sync()
        got = st.cpu().numpy().copy()
        for b in range(2):
            assert np.array_equal(got[b], yards[b][0]), b
        for f in range(n):
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [r[f + 1] for r in raws] if f + 1 < n else None)
            env.sync()
            now = st.cpu().numpy()
            for b in range(2):
                assert np.array_equal(now[b], yards[b][1][f]), (b, f)
    finally:
        end_live(env, st)
        env.ctx.set_batch_clean(None)


# ---- 4. locate
@pytest.mark.parametrize("lanes", [PLAIN, VIEWED], ids=["u16", "view"])
def test_locate_reads_the_cleaned_frame(pool, env, lanes):
    from hpe import locate
    W = env.window
    n = 3
    raws = [pool.raw(v, k)[0] for v, k, _ in lanes]
    cleaned = [pool.frames(*lane)[0] for lane in lanes]
    res = [locate.locate(c[0], FOCAL, unit_mm=1.0) for c in cleaned]
    noisy_res = [locate.locate(pool.raw(v, k)[1][0], FOCAL, unit_mm=1.0) for v, k, _ in lanes]
    assert all(r.found for r in res)
    # the noisy frame locates to something else in at least one lane: the cleaned one was read
    assert any((a.m1, a.m2, tuple(a.px)) != (b.m1, b.m2, tuple(b.px)) for a, b in zip(res, noisy_res))
    T = np.stack([env.x0] * 3)
    T[:, 0] += np.arange(3)
    start = np.stack([env.start()] * 3)
    st = env.batch_states(3, "locate")

    def track(first_rows, init, do_locate, device):
        st.copy_(env.torch.from_numpy(first_rows))
        env.torch.cuda.synchronize()
        env.ctx.set_batch_window("fixed", init, MXY, MZ)
        env.ctx.set_batch_clean([pool.par[p] for _, _, p in lanes] if device else None)
        src = raws if device else cleaned
        kw = begin_kw(pool, lanes) if device else dict(input="u16", unit_mm=1.0, focal=FOCAL)
        out = []
        try:
            env.ctx.batch_pipeline_begin([s[0] for s in src], **kw)
            if do_locate:
                env.ctx.batch_pipeline_locate(st.data_ptr(), T)
                env.sync()
                out.append(st.cpu().numpy().copy())
                out.append([env.ctx.batch_locate_result(b) for b in range(3)])
                out.append([env.ctx.batch_windows_readback(p, 3) for p in (0, 1)])
            for f in range(n):
                env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [s[f + 1] for s in src] if f + 1 < n else None)
                env.sync()
                out.append(st.cpu().numpy().copy())
        finally:
            end_live(env, st)
            env.ctx.set_batch_clean(None)
            env.ctx.set_batch_window("off")
        return out

    a = track(start, [W.WHOLE] * 3, True, True)
    got_rows, results, (w0, w1) = a[0], a[1], a[2]
    rows = []
    for b in range(3):  # every field equals the mirror's on the mirror-cleaned frame
        seq, r = results[b]
        assert seq == 1
        for field in ("found", "k_near", "m1", "m2"):
            assert getattr(r, field) == getattr(res[b], field), (b, field)
        assert np.array_equal(np.array(r.px), np.array(res[b].px))
        assert np.array_equal(np.array(r.centre), np.array(res[b].centre))
        assert tuple(r.window) == tuple(res[b].window)
        S = env.hand.build_batch(T[b])[0][0]
        row = start[b].copy()
        row[:26] = locate.place(locate.camera_centres(S), T[b], res[b].centre)
        rows.append(row)
    rows = np.stack(rows)
    wins = [r.window for r in res]
    assert np.array_equal(got_rows.view(np.uint64), rows.view(np.uint64))
    assert w0 == wins and w1 == wins
    # the tracked frames equal an uncleaned u16 batch on the mirror-cleaned frames, begun with the
    # mirror's windows and rows
    b_ = track(rows, wins, False, False)
    assert np.array_equal(np.array(a[3:]), np.array(b_))
    assert np.isfinite(np.array(b_)).all()


# ---- 5. graphs
def test_parameters_replay_the_graphs_and_off_is_untouched(pool):
    own = pool.other("captures")
    fresh = pool.other("captures fresh")
    n = 3
    for e in (own, fresh):  # the yardsticks first: the single pipeline's first begin starts an epoch
        for lane in PLAIN + [(v, k, "strict") for v, k, _ in PLAIN]:
            e.single(("clean",) + lane, pool.frames(*lane)[1][:n], 1)
    off_q = [pool.noisy[("Q1", s)][:n] for s in range(3)]
    c0 = own.ctx.graph_captures()
    check_clean_lanes(pool, own, PLAIN, n=n, tag="cap")
    c1 = own.ctx.graph_captures()
    assert 1 <= c1 - c0 <= 3
    # other parameters between two batches capture nothing: device memory holds them
    check_clean_lanes(pool, own, [(v, k, "strict") for v, k, _ in PLAIN], n=n, tag="cap")
    assert own.ctx.graph_captures() == c1
    # a batch with cleaning off after one with it on: what a fresh context does, bit for bit and
    # in capture count
    f0 = fresh.ctx.graph_captures()
    want_off = fresh.live(off_q, 1, "u16", 1.0, tag="cap")
    d_fresh = fresh.ctx.graph_captures() - f0
    got_off = own.live(off_q, 1, "u16", 1.0, tag="cap")
    c2 = own.ctx.graph_captures()
    assert c2 - c1 == d_fresh and d_fresh >= 1
    assert np.array_equal(got_off.view(np.uint64), want_off.view(np.uint64))
    # on -> off -> on -> off replays
    check_clean_lanes(pool, own, PLAIN, n=n, tag="cap")
    assert np.array_equal(own.live(off_q, 1, "u16", 1.0, tag="cap").view(np.uint64),
                          want_off.view(np.uint64))
    assert own.ctx.graph_captures() == c2


def test_a_mid_batch_change_applies_from_the_next_frame_cleaned(pool):
    own = pool.other("captures")
    lanes = PLAIN[:2]
    after = ["strict", "default"]
    raws = [pool.raw(v, k)[0] for v, k, _ in lanes]
    # frames 0 and 1 are cleaned before the change (the begin, and call 0's next frames)
    want_u16 = [[pool.par[p if f < 2 else after[b]].apply(pool.raw(v, k)[1][f]) for f in range(NF)]
                for b, (v, k, p) in enumerate(lanes)]
    wants = [own.loop([own.hpe.depth_u16_to_mm(c, 1.0) for c in w], 1) for w in want_u16]
    check_clean_lanes(pool, own, lanes, tag="mid")  # the graphs exist
    c0 = own.ctx.graph_captures()
    st = own.batch_states(2, "mid")
    st.copy_(own.torch.from_numpy(np.stack([own.start(), own.start()])))
    own.torch.cuda.synchronize()
    own.ctx.set_batch_clean([pool.par[p] for _, _, p in lanes])
    try:
        own.ctx.batch_pipeline_begin([r[0].copy() for r in raws], **begin_kw(pool, lanes))
        for f in range(NF):
            own.ctx.track_batch_pipelined(P, 1, st.data_ptr(),
                                          [r[f + 1].copy() for r in raws] if f + 1 < NF else None)
            if f == 0:  # not synchronised first: the call drains the stream itself
                own.ctx.set_batch_clean([pool.par[p] for p in after])
            own.sync()
            now = st.cpu().numpy()
            for b in range(2):
                assert np.array_equal(now[b], wants[b][f]), (b, f)
                if f + 1 < NF:
                    assert np.array_equal(own.ctx.batch_clean_readback((f + 1) & 1, b), want_u16[b][f + 1])
    finally:
        end_live(own, st)
        own.ctx.set_batch_clean(None)
    assert own.ctx.graph_captures() == c0
    assert not np.array_equal(wants[0], own.single(("clean",) + lanes[0], pool.frames(*lanes[0])[1], 1))


# ---- 6. refusals
def test_refusals(pool, env):
    _lib, lib, h = env._lib, env.lib, env.ctx.h
    E_ARG, E_STATE = _lib.HPE_E_ARG, _lib.HPE_E_STATE
    lanes = PLAIN[:2]
    raws = [pool.raw(v, k)[0] for v, k, _ in lanes]
    good = (_lib.CleanPar * 2)(_lib.CleanPar(15, 3, 1, 0), _lib.CleanPar(25, 2, 0, 0))
    arr = (C.c_void_p * 3)(raws[0][0].ctypes.data, raws[1][0].ctypes.data, raws[0][1].ctypes.data)
    fl = [env.hpe.depth_u16_to_mm(r[0], 1.0) for r in raws]
    farr = (C.c_void_p * 2)(fl[0].ctypes.data, fl[1].ctypes.data)
    buf = C.c_void_p()
    out = np.zeros((240, 320), np.uint16)
    op = C.c_void_p(out.ctypes.data)
    st = env.batch_states(2, "refuse")
    assert lib.hpe_set_batch_clean(h, 2, good) == 0
    try:
        # a begin for another lane count, a float begin, a resident float batch
        assert lib.hpe_batch_pipeline_begin_u16(h, 3, arr, 1.0, 1, 1, FOCAL) == E_ARG
        assert lib.hpe_batch_pipeline_begin_u16(h, 1, arr, 1.0, 1, 1, FOCAL) == E_ARG
        assert lib.hpe_batch_pipeline_begin(h, 2, farr, 1, 1, FOCAL) == E_STATE
        d_raw = env.torch.zeros((2, 240 * 320), dtype=env.torch.float32, device="cuda:0")
        parr = (C.c_void_p * 2)(d_raw[0].data_ptr(), d_raw[1].data_ptr())
        assert lib.hpe_track_raw_batch_dev(h, P, 1, 2, C.c_void_p(st.data_ptr()), parr, 1, 1, 1,
                                           FOCAL, 0, None) == E_STATE
        assert lib.hpe_batch_frame_buffer(h, 0, C.byref(buf), None) == E_STATE  # no batch began
        # malformed parameters change nothing
        for bad in (_lib.CleanPar(15, 9, 0, 0), _lib.CleanPar(15, 3, 4, 0), _lib.CleanPar(15, 3, 1, 7)):
            tab = (_lib.CleanPar * 2)(_lib.CleanPar(1, 1, 0, 0), bad)
            assert lib.hpe_set_batch_clean(h, 2, tab) == E_ARG
        assert lib.hpe_set_batch_clean(h, 0, good) == E_ARG
        assert lib.hpe_set_batch_clean(h, 17, good) == E_ARG
        got = check_clean_lanes(pool, env, lanes, n=2)  # the parameters set first still hold
        assert np.isfinite(got).all()
        # during a cleaned batch: off, another lane count and malformed parameters are refused
        assert lib.hpe_set_batch_clean(h, 2, good) == 0
        assert lib.hpe_batch_pipeline_begin_u16(h, 2, arr, 1.0, 1, 1, FOCAL) == 0
        assert lib.hpe_set_batch_clean(h, 0, None) == E_STATE
        assert lib.hpe_set_batch_clean(h, 3, (_lib.CleanPar * 3)()) == E_STATE
        assert lib.hpe_set_batch_clean(h, 2, (_lib.CleanPar * 2)(good[0], _lib.CleanPar(1, 9, 0, 0))) == E_ARG
        assert lib.hpe_set_batch_clean(h, 2, good) == 0
        assert lib.hpe_batch_clean_readback(h, 2, 0, op) == E_ARG
        assert lib.hpe_batch_clean_readback(h, -1, 0, op) == E_ARG
        assert lib.hpe_batch_clean_readback(h, 0, 2, op) == E_ARG
        assert lib.hpe_batch_clean_readback(h, 0, 0, None) == E_ARG
        assert lib.hpe_batch_clean_readback(h, 0, 1, op) == 0
        assert np.array_equal(out, pool.par["loose"].apply(raws[1][0]))
        env.ctx.track_batch_pipelined(P, 0, st.data_ptr(), None)  # the batch ends
        env.sync()
        assert lib.hpe_set_batch_clean(h, 0, None) == 0
        # during an uncleaned batch: turning it on is refused
        assert lib.hpe_batch_pipeline_begin_u16(h, 2, arr, 1.0, 1, 1, FOCAL) == 0
        assert lib.hpe_set_batch_clean(h, 2, good) == E_STATE
        assert lib.hpe_set_batch_clean(h, 0, None) == 0
        env.ctx.track_batch_pipelined(P, 0, st.data_ptr(), None)
        env.sync()
    finally:
        end_live(env, st)
        assert lib.hpe_set_batch_clean(h, 0, None) == 0
    # with cleaning off the float begin works again
    env.ctx.batch_pipeline_begin(fl, input="f32", focal=FOCAL)
    env.ctx.track_batch_pipelined(P, 0, st.data_ptr(), None)
    env.sync()
    check_clean_lanes(pool, env, lanes, n=2)
