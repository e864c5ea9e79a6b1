"""Lane windows (hpe_set_batch_window): every lane of the raw batch and of the live batch reads
its depth frames through a window of its own, fixed or re-centred on the device from the lane's
tracked pose.

The yardstick is always the batch call's single-sequence counterpart -- hpe_track_raw_sequence_dev,
or hpe_pipeline_begin + hpe_track_pipelined -- run on frames masked ON THE HOST by
hpe.window.apply, compared with np.array_equal; never the batch itself.  Under FOLLOW the masks
are built step by step with the single pipelined loop: frame 0 by init, frame 1 by the pose rule
(hpe.window.from_spheres over hpe_build_spheres' centres) on x0, frame g by the rule on the
yardstick's state after frame g-2.

Small shapes: P = 32, maxiter 4 (G = 3), 5 synthetic frames per lane (hpe.synth.trajectory
seeds 0, 1, 2 rendered with render_depth), at most 3 lanes, chunks of 2 frames plus a tail.  One
default context for the file, and one wave-form yardstick context for the wave case.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF, K = 32, 4, 5, 2
FOCAL, MXY, MZ = 241.42, 1.0, 2.0
SENTINEL = -7.0
INF = float("inf")


class Env:
    """One context (created under HPE_PSO_FORM / HPE_PSO_WPP if given) with the single-sequence
    calls -- the yardsticks -- and the batch calls."""

    def __init__(self, form=None, wpp=None, streams=None):
        import hpe
        import torch
        from hpe import _lib, synth, window
        self.hpe, self.torch, self._lib, self.window = hpe, torch, _lib, window
        saved = {k: os.environ.pop(k, None) for k in ("HPE_PSO_FORM", "HPE_PSO_WPP")}
        try:
            if form:
                os.environ["HPE_PSO_FORM"] = form
            if wpp:
                os.environ["HPE_PSO_WPP"] = str(wpp)
            self.hand = hpe.reference_hand(device=0)
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
        if streams is None:
            streams = {}
            for s in range(3):
                streams[s] = [np.ascontiguousarray(self.ctx.render_depth(th), dtype=np.float32)
                              for th in synth.trajectory(NF, s)]
        self.streams = streams
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.h1 = torch.empty((NF, 27), dtype=torch.float64, device="cuda:0")
        self.bufs = {}
        self.cache = {}  # yardsticks: computed once, shared, never changed
        self.sync()

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def start(self, x0=None):
        x = np.zeros(27)
        x[:26] = self.x0 if x0 is None else x0
        return x

    # ---- the pose rule on the host, over hpe_build_spheres' centres
    def rule(self, theta, mxy=MXY, mz=MZ, focal=FOCAL):
        S = self.hand.build_hand_model(np.asarray(theta, dtype=np.float64)[:26])
        return self.window.from_spheres(S, self.radii, focal, mxy, mz)

    # ---- the single-sequence calls
    def pipelined(self, frames, x0=None):
        """hpe_pipeline_begin + hpe_track_pipelined over the frames: the state after every one."""
        n = len(frames)
        self.st1.copy_(self.torch.from_numpy(self.start(x0)))
        self.torch.cuda.synchronize()
        out = []
        self.ctx.pipeline_begin(frames[0])
        for f in range(n):
            self.ctx.track_pipelined(P, 1, self.st1.data_ptr(), frames[f + 1] if f + 1 < n else None)
            self.sync()
            out.append(self.st1.cpu().numpy().copy())
        return np.array(out)

    def raw_alone(self, frames, x0=None):
        """hpe_track_raw_sequence_dev over the frames: (history n x 27, final state)."""
        n = len(frames)
        raw = self.torch.from_numpy(np.stack(frames)).to("cuda:0")
        self.st1.copy_(self.torch.from_numpy(self.start(x0)))
        self.h1.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        self.ctx.track_raw_sequence(P, 1, self.st1.data_ptr(), raw.data_ptr(), n,
                                    frames_per_graph=K, d_hist_ptr=self.h1.data_ptr())
        self.sync()
        return self.h1.cpu().numpy()[:n].copy(), self.st1.cpu().numpy().copy()

    def follow_masks(self, frames, x0, init, mxy=MXY, mz=MZ):
        """FOLLOW's masks, step by step with the single pipelined loop: frame 0 masked by init,
        frame 1 by the rule on x0, frame g by the rule on the loop's state after frame g-2.
        frames: a list, or a function (g, window of frame g) -> frame g, for frames built around
        the very window they will be read through.
        Returns (masked frames, the windows used, the loop's state after every frame, the
        unmasked frames)."""
        x0 = self.x0 if x0 is None else np.asarray(x0, dtype=np.float64)
        n = NF if callable(frames) else len(frames)
        raw = []

        def frame(g, win):
            raw.append(frames(g, win) if callable(frames) else frames[g])
            return raw[g]

        wins = [self.window.as_window(init), self.rule(x0, mxy, mz)]
        masked = [self.window.apply(frame(g, wins[g]), wins[g]) for g in range(min(n, 2))]
        self.st1.copy_(self.torch.from_numpy(self.start(x0)))
        self.torch.cuda.synchronize()
        states = []
        self.ctx.pipeline_begin(masked[0])
        for g in range(n):
            self.ctx.track_pipelined(P, 1, self.st1.data_ptr(), masked[g + 1] if g + 1 < n else None)
            self.sync()
            states.append(self.st1.cpu().numpy().copy())
            if g + 2 < n:
                wins.append(self.rule(states[g], mxy, mz))
                masked.append(self.window.apply(frame(g + 2, wins[-1]), wins[-1]))
        return masked, wins[:n], np.array(states), raw

    def follow_yard(self, name, x0=None, init=None, mxy=MXY, mz=MZ, frames=None):
        """The FOLLOW yardsticks of one stream, cached: dict(masked, wins, states (the pipelined
        loop's), hist and final (the raw sequence call's on the masked frames))."""
        x0 = self.x0 if x0 is None else np.asarray(x0, dtype=np.float64)
        init = self.rule(x0, mxy, mz) if init is None else self.window.as_window(init)
        key = ("follow", name, tuple(x0), tuple(init), mxy, mz)
        if key not in self.cache:
            fr = self.streams[name] if frames is None else frames
            masked, wins, states, raw = self.follow_masks(fr, x0, init, mxy, mz)
            hist, final = self.raw_alone(masked, x0)
            self.cache[key] = dict(masked=masked, wins=wins, states=states, hist=hist, final=final,
                                   init=init, frames=raw)
        return self.cache[key]

    def fixed_yard(self, name, win):
        win = self.window.as_window(win)
        key = ("fixed", name, tuple(win))
        if key not in self.cache:
            masked = [self.window.apply(f, win) for f in self.streams[name]]
            hist, final = self.raw_alone(masked)
            self.cache[key] = dict(masked=masked, hist=hist, final=final,
                                   states=self.pipelined(masked))
        return self.cache[key]

    # ---- the batch calls
    def windows_off(self):
        try:
            self.ctx.set_batch_window("off")
        except self.hpe.HpeError:
            pass  # a live batch a failed test left behind keeps its windows

    def raw_batch(self, raws, mode, init=None, mxy=MXY, mz=MZ, x0s=None, form="auto", tag=None):
        """(history B x n x 27, states B x 27) of hpe_track_raw_batch_dev over device raw
        sequences (tensors n x 240 x 320)."""
        B, n = len(raws), NF
        if (B, tag) not in self.bufs:
            self.bufs[(B, tag)] = (self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0"),
                                   self.torch.empty((B, n, 27), dtype=self.torch.float64, device="cuda:0"))
        st, hist = self.bufs[(B, tag)]
        st.copy_(self.torch.from_numpy(np.stack([self.start(None if x0s is None else x0s[b])
                                                 for b in range(B)])))
        hist.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        self.ctx.set_batch_window(mode, init, mxy, mz)
        self.ctx.set_batch_form(form)
        try:
            self.ctx.track_raw_batch(P, 1, st.data_ptr(), [r.data_ptr() for r in raws], n,
                                     frames_per_graph=K, d_hist_ptr=hist.data_ptr())
            self.sync()
        finally:
            self.ctx.set_batch_form("auto")
            self.windows_off()
        return hist.cpu().numpy(), st.cpu().numpy()

    def live(self, lanes, mode, init=None, mxy=MXY, mz=MZ, x0s=None, form="auto"):
        """The live batch over the lanes' frame lists: (states after every frame n x B x 27, the
        window table read back after every call that prepared a next frame: that frame's
        parity)."""
        B, n = len(lanes), NF
        if (B, "live") not in self.bufs:
            self.bufs[(B, "live")] = self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0")
        st = self.bufs[(B, "live")]
        st.copy_(self.torch.from_numpy(np.stack([self.start(None if x0s is None else x0s[b])
                                                 for b in range(B)])))
        self.torch.cuda.synchronize()
        self.ctx.set_batch_window(mode, init, mxy, mz)
        self.ctx.set_batch_form(form)
        out, tables = [], []
        try:
            self.ctx.batch_pipeline_begin([fr[0] for fr in lanes])
            for f in range(n):
                nxt = [fr[f + 1] for fr in lanes] if f + 1 < n else None
                self.ctx.track_batch_pipelined(P, 1, st.data_ptr(), nxt)
                self.sync()
                out.append(st.cpu().numpy().copy())
                if nxt is not None and mode != "off":
                    tables.append(self.ctx.batch_windows_readback((f + 1) & 1, B))
        finally:
            self.ctx.set_batch_form("auto")
            self.windows_off()
        return np.array(out), tables

    def upload(self, frames):
        return self.torch.from_numpy(np.stack(frames)).to("cuda:0")


class Pool:
    def __init__(self):
        self.env = Env()
        self.raw = {s: self.env.upload(self.env.streams[s]) for s in range(3)}
        self.wave = {}

    def wave_env(self, wpp):
        if wpp not in self.wave:
            self.wave[wpp] = Env("wave", wpp, self.env.streams)
        return self.wave[wpp]

    def close(self):
        self.env.ctx.close()
        for e in self.wave.values():
            e.ctx.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


@pytest.fixture(scope="module")
def env(pool):
    return pool.env


def fixed_windows(env):
    """The three lanes' windows of the FIXED cases: the hand of stream 0 cut roughly in half
    (the left half of x0's window), the whole frame, nothing."""
    w = env.rule(env.x0)
    half = env.window.Window(w.row_lo, w.row_hi, w.col_lo, (w.col_lo + w.col_hi) // 2, w.z_lo, w.z_hi)
    f0 = env.streams[0][0]
    kept = np.count_nonzero(env.window.apply(f0, half))
    assert 0 < kept < np.count_nonzero(f0)  # it does cut the hand
    return [half, env.window.WHOLE, env.window.EMPTY]


# ---- 1. the pose rule on the device
def test_window_from_pose_equals_the_host_rule(env):
    from hpe import synth
    poses = {"x0": env.x0}
    for k, th in enumerate(synth.trajectory(NF, 1)[2:5]):
        poses[f"trajectory {k}"] = th
    for name, dx in (("right edge", 22.0), ("left edge", -22.0), ("out of view", 60.0)):
        th = env.x0.copy()
        th[3] += dx
        poses[name] = th
    up = env.x0.copy()
    up[4] -= 20.0
    poses["row edge"] = up
    nan = env.x0.copy()
    nan[7] = float("nan")
    poses["nan"] = nan
    behind = env.x0.copy()
    behind[5] = -32.0
    poses["behind the camera"] = behind
    for name, th in poses.items():
        for mxy, mz, focal in ((MXY, MZ, FOCAL), (0.0, 0.0, 200.0), (3.5, 0.25, FOCAL)):
            want = env.rule(th, mxy, mz, focal)
            got = env.ctx.window_from_pose(th, focal, mxy, mz)
            assert got == want, (name, mxy, mz, focal, got, want)
    # the cases are what they claim to be (the host rule says so)
    W = env.window
    assert not W.is_whole(env.rule(env.x0))
    assert W.is_whole(env.rule(nan)) and W.is_whole(env.rule(behind))
    r, l, o = env.rule(poses["right edge"]), env.rule(poses["left edge"]), env.rule(poses["out of view"])
    assert (r.col_hi == 319 and r.col_lo > 0) or (r.col_lo == 0 and r.col_hi < 319)
    assert (l.col_hi == 319 and l.col_lo > 0) or (l.col_lo == 0 and l.col_hi < 319)
    assert (o.col_lo, o.col_hi) in ((320, 319), (0, -1))
    u = env.rule(up)
    assert u.row_lo == 0 or u.row_hi == 239


# ---- 2. FIXED
def test_fixed_raw_batch(pool, env):
    wins = fixed_windows(env)
    hist, st = env.raw_batch([pool.raw[0], pool.raw[1], pool.raw[2]], "fixed", wins)
    for b in range(3):
        y = env.fixed_yard(b, wins[b])
        assert np.array_equal(hist[b], y["hist"], equal_nan=(b == 2)), b
        assert np.array_equal(st[b], y["final"], equal_nan=(b == 2)), b
    assert np.isfinite(hist[:2]).all()
    # the lanes in another order give the rows in that order
    order = [2, 0, 1]
    hist2, st2 = env.raw_batch([pool.raw[s] for s in order], "fixed", [wins[s] for s in order])
    for b, s in enumerate(order):
        assert np.array_equal(hist2[b], hist[s], equal_nan=True), (b, s)
        assert np.array_equal(st2[b], st[s], equal_nan=True), (b, s)
    # the half window does change the lane (against the whole-frame window on the same stream)
    assert not np.array_equal(hist[0], env.fixed_yard(0, env.window.WHOLE)["hist"])


def test_fixed_live_batch(env):
    wins = fixed_windows(env)
    got, tables = env.live([env.streams[s] for s in range(3)], "fixed", wins)
    for b in range(3):
        want = env.fixed_yard(b, wins[b])["states"]
        for f in range(NF):
            assert np.array_equal(got[f, b], want[f], equal_nan=(b == 2)), (b, f)
    for t in tables:  # FIXED never rewrites the table
        assert t == [env.window.as_window(w) for w in wins]
    order = [1, 2, 0]
    got2, _ = env.live([env.streams[s] for s in order], "fixed", [wins[s] for s in order])
    for b, s in enumerate(order):
        assert np.array_equal(got2[:, b], got[:, s], equal_nan=True), (b, s)


# ---- 3. FOLLOW, raw batch in chunks of 2 plus a tail
def test_follow_raw_batch(pool, env):
    yards = [env.follow_yard(s) for s in range(3)]
    hist, st = env.raw_batch([pool.raw[s] for s in range(3)], "follow", [y["init"] for y in yards])
    for b, y in enumerate(yards):
        assert np.array_equal(hist[b], y["hist"]), b
        assert np.array_equal(st[b], y["final"]), b
        # the raw sequence call and the pipelined loop agree on the masked frames
        assert np.array_equal(y["hist"], y["states"]), b
    assert np.isfinite(hist).all()
    # the windows do follow: they are not all the first one, and none is the whole frame
    assert any(w != yards[0]["wins"][0] for w in yards[0]["wins"][2:])
    assert not any(env.window.is_whole(w) for y in yards for w in y["wins"])


# ---- 4. FOLLOW, live batch
def test_follow_live_batch(env):
    yards = [env.follow_yard(s) for s in range(3)]
    got, tables = env.live([env.streams[s] for s in range(3)], "follow", [y["init"] for y in yards])
    for b, y in enumerate(yards):
        for f in range(NF):
            assert np.array_equal(got[f, b], y["states"][f]), (b, f)
    # after call k the table of parity (k + 1) & 1 holds the rule on the states call k started
    # from: the yardstick's windows of frame k + 1
    assert len(tables) == NF - 1
    for k, t in enumerate(tables):
        for b, y in enumerate(yards):
            assert t[b] == y["wins"][k + 1], (k, b)


# ---- 5. two hands in one stream
def test_two_hands_in_one_stream(env):
    from hpe import synth
    W = env.window
    found = None
    for d in (7.0, 9.0, 11.0, 13.0):
        poses = [synth.trajectory(NF, 0), synth.trajectory(NF, 1)]
        x0s = [env.x0.copy(), env.x0.copy()]
        for lane, sign in ((0, -1.0), (1, 1.0)):
            poses[lane][:, 3] += sign * d
            x0s[lane][3] += sign * d
        frames = []
        for f in range(NF):
            a = env.ctx.render_depth(poses[0][f])
            b = env.ctx.render_depth(poses[1][f])
            frames.append(np.where((a > 0) & (b > 0), np.minimum(a, b), a + b).astype(np.float32))
        yards = [env.follow_yard(("two hands", d), x0s[b], frames=frames) for b in range(2)]
        lo, hi = (0, 1) if yards[0]["wins"][0].col_lo < yards[1]["wins"][0].col_lo else (1, 0)
        if all(yards[lo]["wins"][g].col_hi < yards[hi]["wins"][g].col_lo for g in range(NF)):
            found = (frames, x0s, yards)
            break
    assert found, "no translation made the two hands' windows column-disjoint"
    frames, x0s, yards = found
    for y in yards:
        assert not any(W.is_whole(w) for w in y["wins"])
        for g in range(NF):  # every mask removes something: the other hand
            kept = np.count_nonzero(y["masked"][g])
            assert 0 < kept < np.count_nonzero(frames[g]), g
    raw = env.upload(frames)  # both lanes name the same buffer
    hist, st = env.raw_batch([raw, raw], "follow", [y["init"] for y in yards], x0s=x0s)
    for b, y in enumerate(yards):
        assert np.array_equal(hist[b], y["hist"]), b
        assert np.array_equal(st[b], y["final"]), b
    assert np.isfinite(hist).all()
    # without windows both lanes see both hands: the case that shows the feature is needed
    hist_off, st_off = env.raw_batch([raw, raw], "off", x0s=x0s)
    for b, y in enumerate(yards):
        assert not np.array_equal(hist_off[b], y["hist"]), b


# ---- 6. FOLLOW under the wave form
def test_follow_raw_batch_wave_form(pool, env):
    wpp = env.ctx.batch_wave_wpp(P, 3)
    assert wpp in (1, 2)
    wenv = pool.wave_env(wpp)
    yards = [wenv.follow_yard(s) for s in range(3)]
    hist, st = env.raw_batch([pool.raw[s] for s in range(3)], "follow", [y["init"] for y in yards],
                             form="wave")
    for b, y in enumerate(yards):
        assert np.array_equal(hist[b], y["hist"]), (b, wpp)
        assert np.array_equal(st[b], y["final"]), (b, wpp)
    assert np.isfinite(hist).all()


# ---- the depth bound, pixel values at the threshold itself
@pytest.mark.parametrize("mode", ["follow", "fixed"])
def test_depth_bound_at_the_threshold(env, mode):
    """A background behind (lane 0) or in front of (lane 1) the hand whose raw values are the
    floats next to the window's own depth bound in raw units -- two below, one below, the nearest
    float, one and two above -- so the depth test decides pixel by pixel, at equality too: against
    z_hi in lane 0, z_lo in lane 1.  Under FOLLOW frame g's background is built around the window
    frame g will be read through (known once the yardstick loop is at frame g-2), so frame 0
    tests the bounds the host wrote and the later frames those the device computed."""
    W = env.window
    f32 = np.float32

    def around(which, base):
        def make(g, win):
            if W.is_whole(win):
                return base[g]
            t = f32((win.z_hi if which == "hi" else win.z_lo) * 10.0)
            dn, up = f32(-np.inf), f32(np.inf)
            vals = np.array([np.nextafter(np.nextafter(t, dn), dn), np.nextafter(t, dn), t,
                             np.nextafter(t, up), np.nextafter(np.nextafter(t, up), up)], f32)
            bg = vals[(3 * np.arange(240)[:, None] + np.arange(320)[None, :]) % 5]
            return np.where(base[g] > 0, base[g], bg).astype(f32)
        return make

    lanes = (("hi", 0), ("lo", 1))
    if mode == "follow":
        yards = [env.follow_yard(("threshold", which), frames=around(which, env.streams[s]))
                 for which, s in lanes]
        init = [y["init"] for y in yards]
    else:
        w = env.rule(env.x0)
        yards = []
        for which, s in lanes:
            frames = [around(which, env.streams[s])(g, w) for g in range(NF)]
            masked = [W.apply(f, w) for f in frames]
            hist, final = env.raw_alone(masked)
            yards.append(dict(frames=frames, masked=masked, hist=hist, final=final, wins=[w] * NF))
        init = [w, w]
    for y, (which, s) in zip(yards, lanes):  # the background straddles the bound in every frame
        for g in range(NF):
            if W.is_whole(y["wins"][g]):
                continue
            wg = y["wins"][g]
            rect = np.zeros((240, 320), bool)
            rect[max(wg.row_lo, 0):wg.row_hi + 1, max(wg.col_lo, 0):wg.col_hi + 1] = True
            bg = (env.streams[s][g] == 0) & rect
            kept = np.count_nonzero(y["masked"][g][bg])
            assert 0 < kept < np.count_nonzero(bg), (which, g)
        assert not W.is_whole(y["wins"][0]) and not W.is_whole(y["wins"][1])
    hist, st = env.raw_batch([env.upload(y["frames"]) for y in yards], mode, init)
    for b, y in enumerate(yards):
        assert np.array_equal(hist[b], y["hist"], equal_nan=True), b
        assert np.array_equal(st[b], y["final"], equal_nan=True), b


# ---- 7. graphs
def test_graphs_are_keyed_by_the_mode_alone(pool, env):
    """The lanes start from a pose 3 cm beside the hand, so that what init and the margins are
    shows in the masks: x0's window with margins (0.5, 2) cuts the hand, the whole frame and the
    margins (6, 2) do not."""
    raws = [pool.raw[1], pool.raw[2]]
    names = (1, 2)
    x0 = env.x0.copy()
    x0[3] += 3.0
    x0s = [x0, x0]
    # every yardstick first: the single-sequence calls capture graphs of their own
    yards = [env.follow_yard(s, x0, mxy=0.5) for s in names]
    y_whole = [env.follow_yard(s, x0, init=env.window.WHOLE, mxy=0.5) for s in names]
    y_wide = [env.follow_yard(s, x0, mxy=6.0) for s in names]
    for b, s in enumerate(names):  # the three runs mask differently (shown on the host)
        fr = env.streams[s]
        assert np.count_nonzero(yards[b]["masked"][0]) < np.count_nonzero(fr[0])
        assert np.array_equal(y_whole[b]["masked"][0], fr[0])
        assert np.count_nonzero(yards[b]["masked"][1]) < np.count_nonzero(y_wide[b]["masked"][1])
    off1 = env.raw_batch(raws, "off", x0s=x0s, tag="graphs")
    c1 = env.ctx.graph_captures()
    fol = env.raw_batch(raws, "follow", [y["init"] for y in yards], 0.5, MZ, x0s=x0s, tag="graphs")
    c2 = env.ctx.graph_captures()
    off2 = env.raw_batch(raws, "off", x0s=x0s, tag="graphs")
    assert env.ctx.graph_captures() == c2  # the first run's graphs replay
    assert c2 > c1                         # FOLLOW captured its own
    assert np.array_equal(off2[0], off1[0]) and np.array_equal(off2[1], off1[1])
    for b, y in enumerate(yards):
        assert np.array_equal(fol[0][b], y["hist"]) and np.array_equal(fol[1][b], y["final"])
    # another init, then other margins: device memory holds them, so both take effect and
    # nothing is captured again; each run equals its own yardstick
    got = env.raw_batch(raws, "follow", [env.window.WHOLE] * 2, 0.5, MZ, x0s=x0s, tag="graphs")
    for b, y in enumerate(y_whole):
        assert np.array_equal(got[0][b], y["hist"]) and np.array_equal(got[1][b], y["final"])
    got = env.raw_batch(raws, "follow", [y["init"] for y in y_wide], 6.0, MZ, x0s=x0s, tag="graphs")
    for b, y in enumerate(y_wide):
        assert np.array_equal(got[0][b], y["hist"]) and np.array_equal(got[1][b], y["final"])
    assert env.ctx.graph_captures() == c2
    # the three FOLLOW runs are three different computations
    for b in range(2):
        assert not np.array_equal(y_whole[b]["hist"], yards[b]["hist"])
        assert not np.array_equal(y_wide[b]["hist"], yards[b]["hist"])


# ---- 8. refusals
def test_refusals_change_nothing(pool, env):
    _lib, lib, h = env._lib, env.lib, env.ctx.h
    M = _lib.BATCH_MAX
    wins = fixed_windows(env)
    arr = (_lib.Window * M)(*([_lib.Window(*w) for w in wins] + [_lib.Window()] * (M - 3)))

    def err():
        return lib.hpe_last_error(h)

    def setw(mode, B, init, mxy=MXY, mz=MZ):
        return lib.hpe_set_batch_window(h, mode, B, init, mxy, mz)

    assert setw(_lib.WINDOW_FIXED, 3, arr) == 0
    for mode in (-1, 3):
        assert setw(mode, 3, arr) == _lib.HPE_E_ARG and b"mode" in err()
    for B in (0, M + 1):
        assert setw(_lib.WINDOW_FOLLOW, B, arr) == _lib.HPE_E_ARG and b"lanes" in err()
    for mode in (_lib.WINDOW_FIXED, _lib.WINDOW_FOLLOW):
        assert setw(mode, 3, None) == _lib.HPE_E_ARG and b"null" in err()
    for bad in (-1.0, float("nan"), INF, -INF):
        assert setw(_lib.WINDOW_FOLLOW, 3, arr, mxy=bad) == _lib.HPE_E_ARG and b"margin" in err()
        assert setw(_lib.WINDOW_FOLLOW, 3, arr, mz=bad) == _lib.HPE_E_ARG and b"margin" in err()
    # a batch call or begin with another lane count than the windows'
    st = env.torch.zeros((3, 27), dtype=env.torch.float64, device="cuda:0")
    st[:, :26] = env.torch.from_numpy(env.x0)
    env.torch.cuda.synchronize()
    raws2 = (C.c_void_p * 2)(pool.raw[0].data_ptr(), pool.raw[1].data_ptr())
    assert lib.hpe_track_raw_batch_dev(h, P, 1, 2, C.c_void_p(st.data_ptr()), raws2, NF, 1, 1, FOCAL,
                                       K, None) == _lib.HPE_E_ARG and b"windows were set for 3" in err()
    f0 = env.streams[0][0]
    fr2 = (C.c_void_p * 2)(f0.ctypes.data, f0.ctypes.data)
    assert lib.hpe_batch_pipeline_begin(h, 2, fr2, 1, 1, FOCAL) == _lib.HPE_E_ARG
    assert b"windows were set for 3" in err()
    # the other two calls' arguments
    w1 = (_lib.Window * M)()
    th = env.x0.ctypes.data_as(_lib.dp)
    assert lib.hpe_window_from_pose(h, None, FOCAL, 1.0, 1.0, w1) == _lib.HPE_E_ARG
    assert lib.hpe_window_from_pose(h, th, FOCAL, 1.0, 1.0, None) == _lib.HPE_E_ARG
    assert lib.hpe_window_from_pose(h, th, 0.0, 1.0, 1.0, w1) == _lib.HPE_E_ARG and b"focal" in err()
    assert lib.hpe_window_from_pose(h, th, FOCAL, -1.0, 1.0, w1) == _lib.HPE_E_ARG and b"margin" in err()
    for parity, B in ((2, 3), (-1, 3), (0, 0), (0, M + 1)):
        assert lib.hpe_batch_windows_readback(h, parity, B, w1) == _lib.HPE_E_ARG
    assert lib.hpe_batch_windows_readback(h, 0, 3, None) == _lib.HPE_E_ARG
    # a live batch in progress keeps what it began with: every set is refused, OFF included
    fr3 = (C.c_void_p * 3)(*[env.streams[s][0].ctypes.data for s in range(3)])
    assert lib.hpe_batch_pipeline_begin(h, 3, fr3, 1, 1, FOCAL) == 0
    assert setw(_lib.WINDOW_OFF, 3, None) == _lib.HPE_E_STATE and b"live batch" in err()
    assert setw(_lib.WINDOW_FOLLOW, 3, arr) == _lib.HPE_E_STATE and b"live batch" in err()
    assert setw(_lib.WINDOW_FIXED, 2, arr) == _lib.HPE_E_STATE and b"live batch" in err()
    # none of the refused calls changed anything: the batch runs to its end under the FIXED
    # windows set first, every lane equal to its yardstick
    for f in range(NF):
        nxt = (C.c_void_p * 3)(*[env.streams[s][f + 1].ctypes.data for s in range(3)]) if f + 1 < NF else None
        assert lib.hpe_track_batch_pipelined(h, P, 1, 3, C.c_void_p(st.data_ptr()), nxt) == 0
        env.sync()
        got = st.cpu().numpy()
        for b in range(3):
            want = env.fixed_yard(b, wins[b])["states"][f]
            assert np.array_equal(got[b], want, equal_nan=(b == 2)), (f, b)
    assert lib.hpe_batch_windows_readback(h, 0, 3, w1) == 0
    assert [env.window.as_window(w1[b]) for b in range(3)] == [env.window.as_window(w) for w in wins]
    assert setw(_lib.WINDOW_OFF, 1, None, 0.0, 0.0) == 0  # the batch has ended
