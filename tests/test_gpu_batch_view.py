"""Lane views: a live batch fed 16-bit frames at the camera's own resolution
(hpe_batch_pipeline_begin_view), the crop, the decimation and the flip done by the preparation's
load, and the lanes' pinned buffers sized to the camera frame (hpe_batch_frame_buffer).

The yardstick is always the single pipelined loop (hpe_pipeline_begin + hpe_track_pipelined) of
one stream alone on hpe.depth_u16_to_mm(view.reduce(camera frame), unit) -- hpe/view.py's numpy
mirror of the rule -- compared with np.array_equal on the 27-double state after EVERY frame;
never a batch.

Camera frames are built from the rendered, quantised 240x320 frames of
tests/test_gpu_batch_input.py: the pixels a view picks hold the rendered values, and EVERY other
camera pixel, the padding columns width..pitch-1 included, holds a non-zero poison that varies
with its position.  A wrong origin, step, pitch or flip then reads garbage, not a neighbouring
copy of the right value.  The inputs are asserted: view.reduce(camera frame) is the rendered
frame (cut where the view leaves the camera image).

Small shapes: P = 64, maxiter 7, at most 4 frames per lane and 3 lanes, but for one 16-lane case
of 2 frames.  One context runs every batch but the capture counts, the wave forms and the lane
hands, which need contexts of their own (as in test_gpu_batch_input.py).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_batch_input import FOCAL, MXY, MZ, P, UHI, Env, follow_yard, quantise

pytestmark = pytest.mark.gpu

NF = 4
UNITS = {"Q1": np.float32(1.0), "Qhi": UHI, "Qhalf": np.float32(0.5)}


def embed(view, model_q, seed=0):
    """The camera frame (height x pitch, uint16) whose picked pixels hold the model frame and
    whose every other pixel -- padding included -- holds a non-zero poison of its position.  The
    model frame is laid out unflipped, as the camera sees it: a flipping view reads it reversed."""
    sr, sc = np.mgrid[0:view.height, 0:view.pitch]
    cam = (1 + (sr * 131 + sc * 17 + seed * 7919) % 60000).astype(np.uint16)
    assert cam.min() >= 1
    plain = type(view)(view.width, view.height, view.pitch, view.row0, view.col0, view.step, 0)
    mr, mc, inside = plain.camera_index()
    cam[mr[inside], mc[inside]] = model_q[inside]
    return np.ascontiguousarray(cam)


class Views:
    """The module's context, rendered streams and views; camera frames and yardsticks are built
    once, shared and never changed."""

    def __init__(self):
        import hpe
        from hpe import synth
        from hpe.view import View
        self.View = View
        self.env = Env()
        e = self.env
        self.render = {s: [np.ascontiguousarray(e.ctx.render_depth(th), dtype=np.float32)
                           for th in synth.trajectory(NF, s)] for s in range(3)}
        self.q = {(u, s): [quantise(r, unit) for r in self.render[s]]
                  for u, unit in UNITS.items() for s in range(3)}
        # where the hand is in stream 0: the cutting views go through it
        rows, cols = np.nonzero(self.q[("Q1", 0)][0])
        self.rmid, self.cmid = int(np.median(rows)), int(np.median(cols))
        self.views = {
            "640x480 step 2": View(640, 480, 640, 0, 0, 2),
            "512x424 step 1": View(512, 424, 512, 92, 96, 1),          # the centred crop
            "848x480 step 2 pitch 896": View(848, 480, 896, 0, 104, 2),
            "1024x1024 step 3 odd origin": View(1024, 1024, 1024, 151, 31, 3),
            "flip": View(640, 480, 672, 0, 0, 2, 1),
            # model rows above the hand's middle and columns left of it lie off the image
            "negative origin": View(640, 480, 640, -2 * self.rmid, -2 * self.cmid, 2),
            # ... and here those below and right of it do
            "past the edges": View(2 * self.cmid + 1, 2 * self.rmid + 1, 2 * self.cmid + 24, 0, 0, 2),
            "outside": View(640, 480, 640, 480, 0, 2),
        }
        self.cam, self.red, self.f = {}, {}, {}
        self.others = {}

    def frames(self, vname, key, n=NF):
        """(camera frames, the float frames of their reduction) of stream `key` under view vname."""
        k = (vname, key)
        if k not in self.cam:
            v = self.views[vname]
            self.cam[k] = [embed(v, q, seed) for seed, q in enumerate(self.q[key])]
            self.red[k] = [v.reduce(c) for c in self.cam[k]]
            want = self.q[key] if not v.flip else [q[:, ::-1] for q in self.q[key]]
            for c, r, q in zip(self.cam[k], self.red[k], want):
                inside = v.camera_index()[2]
                assert np.array_equal(r, np.where(inside, q, 0))  # the inputs are what the case needs
                pad = c[:, v.width:]
                assert (pad != 0).all() and (c != 0).sum() > (r != 0).sum()
            self.f[k] = [self.env.hpe.depth_u16_to_mm(r, UNITS[key[0]]) for r in self.red[k]]
        return self.cam[k][:n], self.f[k][:n]

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
    p = Views()
    yield p
    p.close()


@pytest.fixture(scope="module")
def env(pool):
    return pool.env


def live_view(pool, env, lanes, refine=1, in_place=(), x0s=None, tag=None, n=None):
    """The view batch over lanes = [(view name, stream key)], a frame per lane and call: the
    states after every frame (n x B x 27).  in_place: the lanes whose next frames are written
    into batch_frame_buffer's view and passed back as that view."""
    cams = [pool.frames(v, k)[0][:n] for v, k in lanes]
    views = [pool.views[v] for v, _ in lanes]
    unit = UNITS[lanes[0][1][0]]
    B, n = len(lanes), len(cams[0])
    st = env.batch_states(B, tag)
    st.copy_(env.torch.from_numpy(np.stack([env.start(None if x0s is None else x0s[b])
                                            for b in range(B)])))
    env.torch.cuda.synchronize()
    out = []
    env.ctx.batch_pipeline_begin([c[0].copy() for c in cams], input="view", views=views,
                                 unit_mm=unit, focal=FOCAL)
    for f in range(n):
        nxt = None
        if f + 1 < n:
            nxt = []
            for b, c in enumerate(cams):
                if b in in_place:
                    buf = env.ctx.batch_frame_buffer(b)
                    assert buf.dtype == np.uint16 and buf.shape == (views[b].height, views[b].pitch)
                    buf[:] = c[f + 1]
                    nxt.append(buf)
                else:
                    nxt.append(c[f + 1].copy())
        env.ctx.track_batch_pipelined(P, refine, st.data_ptr(), nxt)
        env.sync()
        out.append(st.cpu().numpy().copy())
    return np.array(out)


def check_view_lanes(pool, env, lanes, refine=1, yard=None, equal_nan=False, n=NF, **kw):
    got = live_view(pool, env, lanes, refine, n=n, **kw)
    for b, (v, k) in enumerate(lanes):
        want = (yard or env).single((v, k), pool.frames(v, k)[1][:n], refine)
        for f in range(n):
            assert np.array_equal(got[f, b], want[f], equal_nan=equal_nan), (v, k, b, f)
    return got


# ---- 1. one view at a time: sizes, steps, origins, pitch
@pytest.mark.parametrize("vname", ["640x480 step 2", "512x424 step 1", "848x480 step 2 pitch 896",
                                   "1024x1024 step 3 odd origin"])
def test_camera_sizes(pool, env, vname):
    v = pool.views[vname]
    assert v.camera_index()[2].all()  # the whole model image lies inside the camera image
    if "odd" in vname:
        assert v.row0 % 2 == 1 and v.col0 % 2 == 1
    got = check_view_lanes(pool, env, [(vname, ("Q1", 0)), (vname, ("Q1", 1))])
    assert np.isfinite(got).all()
    # the reduction is the rendered frame, so the yardstick is the plain u16 stream's
    plain = env.single(("Q1", 0), [env.hpe.depth_u16_to_mm(q, 1.0) for q in pool.q[("Q1", 0)]], 1)
    assert np.array_equal(got[:, 0], plain)


def test_refine_off(pool, env):
    check_view_lanes(pool, env, [("848x480 step 2 pitch 896", ("Q1", 2))], refine=0)


def test_flip(pool, env):
    cam, f = pool.frames("flip", ("Q1", 0))
    for k in range(NF):  # the reduced frame is the column-reversed one, and that is another frame
        rev = pool.q[("Q1", 0)][k][:, ::-1]
        assert np.array_equal(pool.red[("flip", ("Q1", 0))][k], rev)
        assert not np.array_equal(rev, pool.q[("Q1", 0)][k])
    got = check_view_lanes(pool, env, [("flip", ("Q1", 0)), ("640x480 step 2", ("Q1", 0))])
    assert not np.array_equal(got[:, 0], got[:, 1])


@pytest.mark.parametrize("vname", ["negative origin", "past the edges"])
def test_view_leaves_the_image(pool, env, vname):
    _, f = pool.frames(vname, ("Q1", 0))
    inside = pool.views[vname].camera_index()[2]
    assert 0 < inside.sum() < inside.size
    for k in range(NF):  # the cut removes some hand pixels and keeps some
        kept, whole = np.count_nonzero(f[k]), np.count_nonzero(pool.q[("Q1", 0)][k])
        assert 0 < kept < whole, (k, kept, whole)
        assert not f[k][~inside].any()
    got = check_view_lanes(pool, env, [(vname, ("Q1", 0)), ("640x480 step 2", ("Q1", 1))])
    assert not np.array_equal(got[:, 0], env.single(("640x480 step 2", ("Q1", 0)),
                                                    pool.frames("640x480 step 2", ("Q1", 0))[1], 1))


def test_view_wholly_outside_reads_empty_frames(pool, env):
    cam, f = pool.frames("outside", ("Q1", 0))
    assert all((c != 0).all() for c in cam) and not any(x.any() for x in f)
    got = check_view_lanes(pool, env, [("outside", ("Q1", 0)), ("640x480 step 2", ("Q1", 1))],
                           equal_nan=True)
    assert np.isfinite(got[:, 1]).all()


def test_values_above_32767_at_a_fractional_unit(pool, env):
    for q in pool.q[("Qhi", 1)]:
        nz = q[q != 0]
        assert nz.size and nz.min() >= 32768
    check_view_lanes(pool, env, [("1024x1024 step 3 odd origin", ("Qhi", 1)),
                                 ("848x480 step 2 pitch 896", ("Qhi", 2))])
    check_view_lanes(pool, env, [("512x424 step 1", ("Qhalf", 0))])


# ---- 2. several views in one batch
THREE = [("640x480 step 2", ("Q1", 2)), ("848x480 step 2 pitch 896", ("Q1", 1)),
         ("negative origin", ("Q1", 0))]


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_three_views_in_one_batch(pool, env, order):
    lanes = [THREE[k] for k in order]
    got = check_view_lanes(pool, env, lanes)
    views = env.ctx.batch_views_readback(3)
    assert views == [pool.views[v] for v, _ in lanes]  # what was set
    assert not np.array_equal(got[:, 0], got[:, 1])


def test_sixteen_lanes_the_odd_views_at_either_end(pool, env):
    lanes = ([("1024x1024 step 3 odd origin", ("Q1", 0))] +
             [("640x480 step 2", ("Q1", b % 3)) for b in range(1, 15)] + [("flip", ("Q1", 0))])
    got = check_view_lanes(pool, env, lanes, n=2, tag="sixteen")
    assert not np.array_equal(got[:, 0], got[:, 15])
    assert env.ctx.batch_views_readback(16) == [pool.views[v] for v, _ in lanes]


# ---- 3. in place
def test_in_place_delivery(pool, env):
    lanes = [("848x480 step 2 pitch 896", ("Q1", 0)), ("512x424 step 1", ("Q1", 1)),
             ("1024x1024 step 3 odd origin", ("Q1", 2))]
    for in_place in ({0, 1, 2}, {2}):
        check_view_lanes(pool, env, lanes, in_place=in_place)
    # the size is the lane's own camera frame's, and a filled buffer is not copied: the address
    # passed is the buffer's, which the library recognises
    views = [pool.views[v] for v, _ in lanes]
    cams = [pool.frames(v, k)[0] for v, k in lanes]
    st = env.batch_states(3)
    env.ctx.batch_pipeline_begin([c[0] for c in cams], input="view", views=views, unit_mm=1.0)
    addr = []
    for b, v in enumerate(views):
        buf, nb = C.c_void_p(), C.c_size_t(0)
        assert env.lib.hpe_batch_frame_buffer(env.ctx.h, b, C.byref(buf), C.byref(nb)) == 0
        assert nb.value == 2 * v.pitch * v.height
        view_b = env.ctx.batch_frame_buffer(b)
        assert view_b.ctypes.data == buf.value and view_b.nbytes == nb.value
        addr.append(buf.value)
    assert len(set(addr)) == 3
    env.ctx.track_batch_pipelined(P, 0, st.data_ptr(), None)
    env.sync()


# ---- 4. windows, hands, pacing, forms, reports, optimise
def test_fixed_windows(pool, env):
    W = env.window
    w = env.rule(env.x0)
    half = W.Window(w.row_lo, w.row_hi, w.col_lo, (w.col_lo + w.col_hi) // 2, w.z_lo, w.z_hi)
    wins = [half, W.WHOLE]
    lanes = [("848x480 step 2 pitch 896", ("Qhi", 0)), ("512x424 step 1", ("Qhi", 1))]
    fs = [pool.frames(v, k)[1] for v, k in lanes]
    kept = np.count_nonzero(W.apply(fs[0][0], half))
    assert 0 < kept < np.count_nonzero(fs[0][0])  # it does cut the hand
    env.ctx.set_batch_window("fixed", wins, MXY, MZ)
    try:
        got = live_view(pool, env, lanes)
    finally:
        env.ctx.set_batch_window("off")
    for b, (v, k) in enumerate(lanes):
        want = env.single(("fixed", v, k, tuple(wins[b])), [W.apply(f, wins[b]) for f in fs[b]], 1)
        for f in range(NF):
            assert np.array_equal(got[f, b], want[f]), (b, f)
    assert not np.array_equal(got[:, 0], env.single(lanes[0], fs[0], 1))


def test_follow_windows(pool, env):
    lanes = [("1024x1024 step 3 odd origin", ("Qhi", 0)), ("flip", ("Qhi", 1))]
    fs = [pool.frames(v, k)[1] for v, k in lanes]
    x0s = [env.x0, env.x0]
    inits = [env.rule(x) for x in x0s]
    yards = [follow_yard(env, fs[b], x0s[b], inits[b]) for b in range(2)]
    env.ctx.set_batch_window("follow", inits, MXY, MZ)
    try:
        got = live_view(pool, env, lanes, x0s=x0s)
    finally:
        env.ctx.set_batch_window("off")
    for b in range(2):
        for f in range(NF):
            assert np.array_equal(got[f, b], yards[b][1][f]), (b, f)


def test_lane_hands(pool, env):
    scales = [(0.9, 0.85), (1.1, 1.2)]
    lanes = [("848x480 step 2 pitch 896", ("Q1", 1)), ("512x424 step 1", ("Q1", 2))]
    yards = [pool.other(("hand", s), hand=s) for s in scales]
    env.ctx.set_batch_hands([y.hand for y in yards])
    try:
        got = live_view(pool, env, lanes, tag="hands", n=3)
    finally:
        env.ctx.set_batch_hands(None)
    for b, (v, k) in enumerate(lanes):
        f3 = pool.frames(v, k)[1][:3]
        want = yards[b].single((v, k), f3, 1)
        for f in range(3):
            assert np.array_equal(got[f, b], want[f]), (b, f)
        assert not np.array_equal(got[:, b], env.single((v, k), f3, 1))


def test_free_pacing_with_a_late_joiner(pool, env):
    torch = env.torch
    lanes = [("640x480 step 2", ("Q1", 0)), ("848x480 step 2 pitch 896", ("Q1", 1)),
             ("1024x1024 step 3 odd origin", ("Q1", 2))]
    views = [pool.views[v] for v, _ in lanes]
    cams = [pool.frames(v, k)[0] for v, k in lanes]
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
            fr[b] = cams[b][took[b]].copy()
            took[b] += 1
        return fr

    env.ctx.set_batch_pacing("free")
    try:
        env.ctx.batch_pipeline_begin(frames(sched[0]), input="view", views=views, unit_mm=1.0)
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
        env.sync()
        env.ctx.set_batch_pacing("lockstep")
    assert [len(t) for t in tracked] == [4, 3, 3] == took
    for b, (v, k) in enumerate(lanes):
        want = env.single((v, k), pool.frames(v, k)[1][:took[b]], 1)
        for f in range(took[b]):
            assert np.array_equal(tracked[b][f], want[f]), (b, f)


@pytest.mark.parametrize("wpp", [1, 2])
def test_wave_form(pool, wpp):
    lanes = [("848x480 step 2 pitch 896", ("Q1", 1)), ("flip", ("Q1", 2))]
    own = pool.other(("wpp", wpp), wpp=wpp)  # a batch context that only forces the waves per particle
    assert own.ctx.batch_wave_wpp(P, 2) == wpp
    yard = pool.other(("wave", wpp), form="wave", wpp=wpp)
    own.ctx.set_batch_form("wave")
    try:
        got = check_view_lanes(pool, own, lanes, yard=yard, n=3)
    finally:
        own.ctx.set_batch_form("auto")
    assert np.isfinite(got).all()


def test_reports_equal_the_non_view_batch(pool, env):
    lanes = [("1024x1024 step 3 odd origin", ("Q1", 0)), ("past the edges", ("Q1", 0))]
    n = 3

    def run(view):
        st = env.batch_states(2, "report")
        st.copy_(env.torch.from_numpy(np.stack([env.start(), env.start()])))
        env.torch.cuda.synchronize()
        src = [pool.frames(v, k)[0] if view else pool.red[(v, k)] for v, k in lanes]
        kw = dict(input="view", views=[pool.views[v] for v, _ in lanes]) if view else dict(input="u16")
        reps = []
        env.ctx.set_batch_report(4)
        try:
            env.ctx.batch_pipeline_begin([s[0] for s in src], unit_mm=1.0, **kw)
            for f in range(n):
                env.ctx.track_batch_pipelined(P, 1, st.data_ptr(),
                                              [s[f + 1] for s in src] if f + 1 < n else None)
                env.sync()
                reps.append([env.ctx.batch_report(b, raw=True) for b in range(2)])
        finally:
            env.sync()
            env.ctx.set_batch_report(0)
        return reps

    for v, k in lanes:
        pool.frames(v, k)
    a, b_ = run(True), run(False)
    for f in range(n):
        for lane in range(2):
            x, y = a[f][lane], b_[f][lane]
            assert (x.seq, x.kind, x.n, x.flags) == (y.seq, y.kind, y.n, y.flags) and x.seq == f + 1
            for field in ("state", "joints", "px"):
                assert np.array_equal(np.array(getattr(x, field)), np.array(getattr(y, field))), (f, lane, field)
            want = env.single(lanes[lane], pool.frames(*lanes[lane])[1][:n], 1)[f]
            assert np.array_equal(np.array(x.state), want)
    # report pixels are model pixels: the view maps them back into the camera image
    v = pool.views[lanes[0][0]]
    px = np.array(a[0][0].px)
    cam_px = v.to_camera(px)
    assert np.allclose(cam_px, [v.col0, v.row0] + 3.0 * px) and np.allclose(v.to_model(cam_px), px)


def test_batch_pipeline_optimise(pool, env):
    lanes = [("848x480 step 2 pitch 896", ("Q1", 1)), ("negative origin", ("Q1", 0))]
    n, G = 2, 6
    yards = []
    for b, (v, k) in enumerate(lanes):  # the single call on the reduced frame, then the single loop
        f = pool.frames(v, k)[1]
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
    cams = [pool.frames(v, k)[0] for v, k in lanes]
    env.ctx.batch_pipeline_begin([c[0] for c in cams], input="view",
                                 views=[pool.views[v] for v, _ in lanes], unit_mm=1.0)
    env.ctx.batch_pipeline_optimise(P, st.data_ptr())
    env.sync()
    got = st.cpu().numpy().copy()
    for b in range(2):
        assert np.array_equal(got[b], yards[b][0]), b
    for f in range(n):
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [c[f + 1] for c in cams] if f + 1 < n else None)
        env.sync()
        now = st.cpu().numpy()
        for b in range(2):
            assert np.array_equal(now[b], yards[b][1][f]), (b, f)


# ---- 5. locate
def test_locate_reads_through_the_view(pool, env):
    from hpe import locate
    W = env.window
    lanes = [("1024x1024 step 3 odd origin", ("Qhalf", 0)), ("flip", ("Qhalf", 1)),
             ("outside", ("Qhalf", 2))]
    unit, n = UNITS["Qhalf"], 3
    views = [pool.views[v] for v, _ in lanes]
    cams = [pool.frames(v, k)[0] for v, k in lanes]
    reds = [pool.red[(v, k)] for v, k in lanes]
    res = [locate.locate(r[0], FOCAL, unit_mm=unit) for r in reds]
    assert [r.found for r in res] == [1, 1, 0]
    T = np.stack([env.x0] * 3)
    T[:, 0] += np.arange(3)
    start = np.stack([env.start()] * 3)

    def placed(b):
        if not res[b].found:
            return start[b].copy()
        S = env.hand.build_batch(T[b])[0][0]
        out = start[b].copy()
        out[:26] = locate.place(locate.camera_centres(S), T[b], res[b].centre)
        return out

    rows = np.stack([placed(b) for b in range(3)])
    wins = [r.window if r.found else W.WHOLE for r in res]
    st = env.batch_states(3, "locate")

    def track(first_rows, init, do_locate):
        st.copy_(env.torch.from_numpy(first_rows))
        env.torch.cuda.synchronize()
        env.ctx.set_batch_window("fixed", init, MXY, MZ)
        out = []
        try:
            env.ctx.batch_pipeline_begin([c[0] for c in cams], input="view", views=views, unit_mm=unit)
            if do_locate:
                env.ctx.batch_pipeline_locate(st.data_ptr(), T)
                env.sync()
                out.append(st.cpu().numpy().copy())
                out.append([env.ctx.batch_locate_result(b) for b in range(3)])
                out.append([env.ctx.batch_windows_readback(p, 3) for p in (0, 1)])
            for f in range(n):
                env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [c[f + 1] for c in cams] if f + 1 < n else None)
                env.sync()
                out.append(st.cpu().numpy().copy())
        finally:
            env.sync()
            env.ctx.set_batch_window("off")
        return out

    a = track(start, [W.WHOLE] * 3, True)
    got_rows, results, (w0, w1) = a[0], a[1], a[2]
    for b in range(3):  # every field equals the mirror's on the reduced frame
        seq, r = results[b]
        assert seq == 1
        for field in ("found", "k_near", "m1", "m2"):
            assert getattr(r, field) == getattr(res[b], field), (b, field)
        assert np.array_equal(np.array(r.px), np.array(res[b].px))
        assert np.array_equal(np.array(r.centre), np.array(res[b].centre))
        assert tuple(r.window) == tuple(res[b].window)
    assert np.array_equal(got_rows.view(np.uint64), rows.view(np.uint64))
    assert w0 == wins and w1 == wins
    # the tracked frames equal a batch begun with the mirror's windows and rows
    b_ = track(rows, wins, False)
    assert np.array_equal(np.array(a[3:]), np.array(b_), equal_nan=True)
    assert np.isfinite(np.array(b_)[:, :2]).all()
    # a located centre is a model pixel: back in the camera image through the view
    v = views[0]
    assert np.allclose(v.to_camera(res[0].px), [v.col0 + 3 * res[0].px[0], v.row0 + 3 * res[0].px[1]])


# ---- 6. graphs, formats in turn, refusals
def test_other_views_replay_the_same_graphs(pool):
    own = pool.other("captures")
    a_l = [("640x480 step 2", ("Q1", 0)), ("512x424 step 1", ("Q1", 1))]
    b_l = [("848x480 step 2 pitch 896", ("Q1", 0)), ("1024x1024 step 3 odd origin", ("Q1", 2))]
    for v, k in a_l + b_l:  # the yardsticks first: the single pipeline's first begin starts an epoch
        own.single((v, k), pool.frames(v, k)[1][:3], 1)
    c0 = own.ctx.graph_captures()
    check_view_lanes(pool, own, a_l, n=3, tag="views")
    c1 = own.ctx.graph_captures()
    assert 1 <= c1 - c0 <= 3
    check_view_lanes(pool, own, b_l, n=3, tag="views")  # larger frames: the buffers grow, too
    assert own.ctx.graph_captures() == c1  # the views are device memory, not part of any graph


def test_float_u16_view_u16_in_turn_on_one_context(pool):
    own = pool.other("turns")
    n = 3
    q = [pool.q[("Q1", s)][:n] for s in range(2)]
    f = [[own.hpe.depth_u16_to_mm(x, 1.0) for x in q[s]] for s in range(2)]
    want = [own.single(("Q1", s), f[s], 1) for s in range(2)]
    lanes = [("1024x1024 step 3 odd origin", ("Q1", 0)), ("848x480 step 2 pitch 896", ("Q1", 1))]

    def same(got):
        for b in range(2):
            for k in range(n):
                assert np.array_equal(got[k, b], want[b][k]), (b, k)

    same(own.live(f, 1, "f32", tag="turns"))
    same(own.live(q, 1, "u16", 1.0, tag="turns"))
    same(live_view(pool, own, lanes, n=n, tag="turns"))
    same(own.live(q, 1, "u16", 1.0, in_place={0, 1}, tag="turns"))  # Env.live asserts 240x320 buffers
    same(live_view(pool, own, lanes, n=n, tag="turns", in_place={0, 1}))
    same(own.live(f, 1, "f32", tag="turns", in_place={0}))
    # hpe_track_batch_pipelined (float) on a view batch is refused, as on a u16 batch
    cams = [pool.frames(v, k)[0] for v, k in lanes]
    st = own.batch_states(2, "turns")
    own.ctx.batch_pipeline_begin([c[0] for c in cams], input="view",
                                 views=[pool.views[v] for v, _ in lanes], unit_mm=1.0)
    fa = (C.c_void_p * 2)(f[0][1].ctypes.data, f[1][1].ctypes.data)
    rc = own.lib.hpe_track_batch_pipelined(own.ctx.h, P, 1, 2, C.c_void_p(st.data_ptr()), fa)
    assert rc == own._lib.HPE_E_STATE
    own.ctx.track_batch_pipelined(P, 0, st.data_ptr(), None)
    own.sync()


BAD = [("null views", None), ("step 0", dict(step=0)), ("step 9", dict(step=9)),
       ("width 0", dict(width=0)), ("height 0", dict(height=0)), ("pitch < width", dict(pitch=639)),
       ("pitch > 2048", dict(width=2049, pitch=2049, height=8)),
       ("height > 2048", dict(width=8, pitch=8, height=2049)),
       ("too many pixels", dict(width=2048, pitch=2048, height=1025)),
       ("unknown flag", dict(flags=2)), ("pad", dict(pad=1))]


@pytest.mark.parametrize("what,bad", BAD)
def test_refusals_leave_the_context_usable(pool, env, what, bad):
    _lib, lib, h = env._lib, env.lib, env.ctx.h
    lanes = [("640x480 step 2", ("Q1", 0)), ("512x424 step 1", ("Q1", 1))]
    cams = [pool.frames(v, k)[0] for v, k in lanes]
    good = [pool.views[v] for v, _ in lanes]
    check_view_lanes(pool, env, lanes, n=2)  # a batch ran and ended; its views are in the table
    fields = dict(width=640, height=480, pitch=640, row0=0, col0=0, step=2, flags=0, pad=0)
    big = np.zeros(2048 * 1025 + 2049 * 8, np.uint16)  # no refusal depends on reading a frame
    arr = (C.c_void_p * 2)(cams[0][0].ctypes.data, big.ctypes.data)
    if bad is None:
        tab = None
    else:
        fields.update(bad)
        tab = (_lib.View * 2)(_lib.View(*[getattr(good[0], f) for f in
                                          ("width", "height", "pitch", "row0", "col0", "step", "flags", "pad")]),
                              _lib.View(*[fields[f] for f in
                                          ("width", "height", "pitch", "row0", "col0", "step", "flags", "pad")]))
    rc = lib.hpe_batch_pipeline_begin_view(h, 2, arr, tab, 1.0, 1, 1, FOCAL)
    assert rc == _lib.HPE_E_ARG, what
    assert env.ctx.batch_views_readback(2) == good  # nothing changed
    buf = C.c_void_p()
    assert lib.hpe_batch_frame_buffer(h, 0, C.byref(buf), None) == _lib.HPE_E_STATE  # no batch began
    check_view_lanes(pool, env, lanes, n=2)  # and the context goes on


def test_other_refusals(pool, env):
    _lib, lib, h = env._lib, env.lib, env.ctx.h
    v = pool.views["640x480 step 2"]
    cam = pool.frames("640x480 step 2", ("Q1", 0))[0][0]
    arr = (C.c_void_p * 1)(cam.ctypes.data)
    tab = (_lib.View * 1)(_lib.View(v.width, v.height, v.pitch, v.row0, v.col0, v.step, v.flags, 0))
    for unit in (0.0, -1.0, float("nan"), float("inf")):  # the u16 begin's refusals
        assert lib.hpe_batch_pipeline_begin_view(h, 1, arr, tab, unit, 1, 1, FOCAL) == _lib.HPE_E_ARG
    assert lib.hpe_batch_pipeline_begin_view(h, 0, arr, tab, 1.0, 1, 1, FOCAL) == _lib.HPE_E_ARG
    assert lib.hpe_batch_pipeline_begin_view(h, 1, None, tab, 1.0, 1, 1, FOCAL) == _lib.HPE_E_ARG
    assert lib.hpe_batch_pipeline_begin_view(h, 1, arr, tab, 1.0, 1, 0, FOCAL) == _lib.HPE_E_ARG
    assert lib.hpe_batch_pipeline_begin_view(h, 1, arr, tab, 1.0, 1, 1, 0.0) == _lib.HPE_E_ARG
    out = (_lib.View * 16)()
    assert lib.hpe_batch_views_readback(h, 0, out) == _lib.HPE_E_ARG
    assert lib.hpe_batch_views_readback(h, 1, None) == _lib.HPE_E_ARG
    fresh = pool.other("fresh")  # no view batch has begun there
    assert fresh.lib.hpe_batch_views_readback(fresh.ctx.h, 1, out) == _lib.HPE_E_STATE
    check_view_lanes(pool, env, [("640x480 step 2", ("Q1", 0))], n=2)
