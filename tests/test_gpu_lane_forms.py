"""The live batch in every combination of its settings that no other test runs:
{f32, u16 frames} x {windows off, fixed, follow} x {lockstep, free pacing} x {the context's hand,
lane hands} x {auto, wave form} x {hand-frame, exact refine}.  COVERED lists the combinations the
feature tests run, with the test that runs each; the cases here are all the others.  The raw
batch's {windows} x {hands} x {form} x {refine} likewise (RAW_COVERED, test_raw_batch), and the
prepared batch's {hands} x {form} x {refine} (PREPARED_COVERED, test_prepared_batch).
tests/test_lane_forms_coverage.py checks that every test the three maps name exists.

The yardstick of the live and the raw batch is always the single pipelined loop
(hpe_pipeline_begin + hpe_track_pipelined) of one stream alone, on a context created with the
lane's hand (under HPE_PSO_FORM=wave and the batch's waves per particle for the wave form) and set
to the batch's refine form, over the float frames masked on the host (hpe/window.py) by the window
the lane read them through -- init[b] for a frame given at the begin and under "fixed", the pose
rule on the lane's row before the call that accepted the frame under "follow" -- compared with
np.array_equal on the 27-double state after EVERY frame; never a batch.  The prepared batch's is
hpe_track_sequence_dev of the lane alone on such a context, as in tests/test_gpu_batch.py.

Without windows lane b tracks stream b (hpe.synth.trajectory seed b).  With windows both lanes
read ONE stream that holds two hands, 9 cm to either side, lane b starting at and following hand
b: every window must cut the other hand away.  That is asserted on every frame (the mask removes
pixels and keeps some), the result must differ from the same stream tracked without windows, and
under "follow" the device's window tables are read back and compared with the host rule.

Small shapes: P = 64, maxiter 7, 2 lanes, 3 frames per lane.  The 16-bit frames are the rendered
ones quantised at 0.0055 mm per count (every non-zero pixel above 32767), the float frames their
conversion (hpe.depth_u16_to_mm): both inputs share a yardstick.  Under free pacing lane 1 is
given no frame in the first call and so skips the second.
"""
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF = 64, 7, 3
FOCAL, MXY, MZ = 241.42, 1.0, 2.0
UNIT = np.float32(0.0055)
APART = 9.0  # cm: the two hands of the windowed stream sit at x -/+ APART
SCALES = [(0.9, 0.85), (1.1, 1.2)]  # the lane hands
# the lanes given a frame at the begin and by every call (None: the last call)
SCHED = {"lockstep": [{0, 1}, {0, 1}, {0, 1}, None],
         "free": [{0, 1}, {0}, {0, 1}, {1}, None]}

AXES = (("f32", "u16"), ("off", "fixed", "follow"), ("lockstep", "free"), ("shared", "lane"),
        ("auto", "wave"), ("rigid", "exact"))
# (input, window, pacing, hands, form, refine) -> the test that runs it
COVERED = {
    ("f32", "off", "lockstep", "shared", "auto", "rigid"): "test_gpu_batch_live::test_three_lanes_six_frames",
    ("f32", "off", "lockstep", "shared", "auto", "exact"): "test_gpu_batch_live::test_both_refine_forms[True]",
    ("f32", "off", "lockstep", "shared", "wave", "rigid"):
        "test_gpu_batch_wave::test_live_batch_and_a_form_change_inside_it",
    ("f32", "off", "lockstep", "lane", "auto", "rigid"): "test_gpu_batch_hands::test_three_hands[live-1]",
    ("f32", "off", "lockstep", "lane", "wave", "rigid"): "test_gpu_batch_hands::test_wave_form[live-2]",
    ("f32", "fixed", "lockstep", "shared", "auto", "rigid"): "test_gpu_batch_window::test_fixed_live_batch",
    ("f32", "follow", "lockstep", "shared", "auto", "rigid"): "test_gpu_batch_window::test_follow_live_batch",
    ("f32", "off", "free", "shared", "auto", "rigid"): "test_gpu_batch_pacing::test_gaps[1]",
    ("f32", "off", "free", "shared", "wave", "rigid"): "test_gpu_batch_pacing::test_wave_form[2]",
    ("f32", "off", "free", "shared", "auto", "exact"): "test_gpu_batch_pacing::test_both_refine_forms[True]",
    ("f32", "follow", "free", "lane", "auto", "rigid"):
        "test_gpu_batch_pacing::test_windows_with_lane_hands_and_gaps[follow]",
    ("f32", "fixed", "free", "lane", "auto", "rigid"):
        "test_gpu_batch_pacing::test_windows_with_lane_hands_and_gaps[fixed]",
    ("u16", "off", "lockstep", "shared", "auto", "rigid"): "test_gpu_batch_input::test_three_lanes_five_frames",
    ("u16", "fixed", "lockstep", "shared", "auto", "rigid"): "test_gpu_batch_input::test_fixed_windows",
    ("u16", "follow", "lockstep", "shared", "auto", "rigid"): "test_gpu_batch_input::test_follow_windows",
    ("u16", "off", "free", "shared", "auto", "rigid"): "test_gpu_batch_input::test_free_pacing",
    ("u16", "off", "lockstep", "shared", "wave", "rigid"): "test_gpu_batch_input::test_wave_form",
    ("u16", "off", "lockstep", "lane", "auto", "rigid"): "test_gpu_batch_input::test_lane_hands",
}
CASES = [c for c in itertools.product(*AXES) if c not in COVERED]

# The raw batch (hpe_track_raw_batch_dev: float frames, no pacing): (window, hands, form, refine)
RAW_COVERED = {
    ("off", "shared", "auto", "rigid"): "test_gpu_batch_raw::test_three_lanes_chunk_and_tail",
    ("off", "shared", "auto", "exact"): "test_gpu_batch_raw::test_both_refine_forms[True]",
    ("off", "shared", "wave", "rigid"): "test_gpu_batch_wave::test_raw_batch",
    ("fixed", "shared", "auto", "rigid"): "test_gpu_batch_window::test_fixed_raw_batch",
    ("follow", "shared", "auto", "rigid"): "test_gpu_batch_window::test_follow_raw_batch",
    ("follow", "shared", "wave", "rigid"): "test_gpu_batch_window::test_follow_raw_batch_wave_form",
    ("off", "lane", "auto", "rigid"): "test_gpu_batch_hands::test_three_hands[raw-1]",
    ("off", "lane", "wave", "rigid"): "test_gpu_batch_hands::test_wave_form[raw-2]",
    ("follow", "lane", "auto", "rigid"): "test_gpu_batch_hands::test_follow_windows_with_lane_hands",
}
RAW_CASES = [c for c in itertools.product(AXES[1], AXES[3], AXES[4], AXES[5]) if c not in RAW_COVERED]

# The prepared batch (hpe_track_batch_dev: stored slots, no preparation): (hands, form, refine)
PREPARED_COVERED = {
    ("shared", "auto", "rigid"): "test_gpu_batch::test_three_lanes_chunk_and_tail",
    ("shared", "auto", "exact"): "test_gpu_batch::test_both_refine_forms[True]",
    ("shared", "wave", "rigid"): "test_gpu_batch_wave::test_tail_waves_chunk_and_tail",
    ("lane", "auto", "rigid"): "test_gpu_batch_hands::test_three_hands[prepared-1]",
}
PREPARED_CASES = [c for c in itertools.product(AXES[3], AXES[4], AXES[5]) if c not in PREPARED_COVERED]
SLOT0 = (10, 20)  # the two lanes' first slots


class Env:
    """One context on hand `hand` (default: the reference hand; created under HPE_PSO_FORM /
    HPE_PSO_WPP if given) with the single pipelined loop, the yardstick."""

    def __init__(self, hand=None, form=None, wpp=None):
        import hpe
        import torch
        from hpe import window
        self.hpe, self.torch, self.window = hpe, torch, window
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
        ub, lb, sd = hpe.reference_bounds()
        self.pso = hpe.PSO()
        self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        self.pso._push(self.ctx)
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        self.radii = np.asarray(self.hand.spheres_radii, dtype=np.float64)
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.h1 = torch.empty((NF, 27), dtype=torch.float64, device="cuda:0")
        self._single = {}  # yardsticks: computed once, shared, never changed
        self.stored = False
        self.sync()

    def sync(self):
        self.ctx.check(self.ctx.lib.hpe_sync(self.ctx.h))

    def start(self, x0=None):
        x = np.zeros(27)
        x[:26] = self.x0 if x0 is None else np.asarray(x0)[:26]
        return x

    def rule(self, theta):
        S = self.hand.build_hand_model(np.asarray(theta, dtype=np.float64)[:26])
        return self.window.from_spheres(S, self.radii, FOCAL, MXY, MZ)

    def loop(self, frames, exact, x0=None):
        """The single pipelined loop over float frames, refine on: the state after every frame."""
        n = len(frames)
        self.ctx.refine_exact = exact
        try:
            self.st1.copy_(self.torch.from_numpy(self.start(x0)))
            self.torch.cuda.synchronize()
            out = []
            self.ctx.pipeline_begin(frames[0])
            for f in range(n):
                self.ctx.track_pipelined(P, 1, self.st1.data_ptr(), frames[f + 1] if f + 1 < n else None)
                self.sync()
                out.append(self.st1.cpu().numpy().copy())
        finally:
            self.ctx.refine_exact = False
        return np.array(out)

    def single(self, key, frames, exact, x0=None):
        if key not in self._single:
            self._single[key] = self.loop(frames, exact, x0)
        return self._single[key]

    def store(self, lanes):
        """Lane b's frames into slots SLOT0[b].. of this context (once)."""
        if not self.stored:
            for b, fr in enumerate(lanes):
                for f, d in enumerate(fr):
                    self.ctx.prepare_frame(SLOT0[b] + f, d)
            self.sync()
            self.stored = True

    def sequence(self, slot0, exact):
        """hpe_track_sequence_dev of one lane alone, refine on: (history NF x 27, final state)."""
        key = ("sequence", slot0, exact)
        if key not in self._single:
            self.ctx.refine_exact = exact
            try:
                self.st1.copy_(self.torch.from_numpy(self.start()))
                self.h1.fill_(np.nan)
                self.torch.cuda.synchronize()
                self.ctx.track_sequence(P, 1, self.st1.data_ptr(), slot0, NF, 2, self.h1.data_ptr())
                self.sync()
                self._single[key] = (self.h1.cpu().numpy().copy(), self.st1.cpu().numpy().copy())
            finally:
                self.ctx.refine_exact = False
        return self._single[key]


class Pool:
    def __init__(self):
        from hpe import synth
        self.env = Env()
        e = self.env
        self.q = [[self.quantise(e.ctx.render_depth(th)) for th in synth.trajectory(NF, s)]
                  for s in range(2)]
        self.f = [[e.hpe.depth_u16_to_mm(q, UNIT) for q in lane] for lane in self.q]
        # the windowed stream: both hands in every frame, hand b at x -/+ APART
        poses = [synth.trajectory(NF, 0), synth.trajectory(NF, 1)]
        self.x0s = [e.x0.copy(), e.x0.copy()]
        for b, sign in ((0, -1.0), (1, 1.0)):
            poses[b][:, 3] += sign * APART
            self.x0s[b][3] += sign * APART
        self.q2 = []
        for f in range(NF):
            a, b = e.ctx.render_depth(poses[0][f]), e.ctx.render_depth(poses[1][f])
            self.q2.append(self.quantise(np.where((a > 0) & (b > 0), np.minimum(a, b), a + b)))
        self.f2 = [e.hpe.depth_u16_to_mm(q, UNIT) for q in self.q2]
        self.states = e.torch.zeros((2, 27), dtype=e.torch.float64, device="cuda:0")
        self.hist = e.torch.empty((2, NF, 27), dtype=e.torch.float64, device="cuda:0")
        self.raw = [e.torch.from_numpy(np.stack(f)).to("cuda:0") for f in self.f]
        self.raw2 = e.torch.from_numpy(np.stack(self.f2)).to("cuda:0")
        self.yards = {("shared", "auto"): [e, e]}

    @staticmethod
    def quantise(render):
        q = np.rint(np.asarray(render, dtype=np.float32) / UNIT)
        assert q.min() >= 0 and q.max() <= 65535
        q = np.ascontiguousarray(q.astype(np.uint16))
        nz = q[q != 0]
        assert nz.size and nz.min() >= 32768
        return q

    def yard(self, hands, form, wpp):
        """The two lanes' yardstick contexts"""
        if (hands, form) not in self.yards:
            kw = dict(form="wave", wpp=wpp) if form == "wave" else {}
            if hands == "shared":
                e = Env(**kw)
                self.yards[(hands, form)] = [e, e]
            else:
                self.yards[(hands, form)] = [Env(hand=s, **kw) for s in SCALES]
        return self.yards[(hands, form)]

    def streams(self, window, u16=False):
        """(the two lanes' frame lists as fed, as float frames, the lanes' start poses)"""
        if window == "off":
            return (self.q if u16 else self.f), self.f, [self.env.x0, self.env.x0]
        two = self.q2 if u16 else self.f2
        return [two, two], [self.f2, self.f2], self.x0s

    def check_windows(self, y, b, exact, wins, got):
        """Lane b's windowed yardstick: the two-hand frames masked by `wins` on the host.  Every
        mask removes pixels (the other hand) and keeps some, and what the lane computed is not
        what the unwindowed stream gives."""
        W = self.env.window
        masked = [W.apply(f, w) for f, w in zip(self.f2, wins)]
        for f, m in zip(self.f2, masked):
            assert 0 < np.count_nonzero(m) < np.count_nonzero(f), b
        unwindowed = y.single(("two hands", b, exact), self.f2, exact, self.x0s[b])
        assert not np.array_equal(np.asarray(got), unwindowed, equal_nan=True), b
        return y.loop(masked, exact, self.x0s[b])

    def close(self):
        for e in {id(e): e for pair in self.yards.values() for e in pair}.values():
            e.ctx.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


def run_batch(pool, input, window, pacing, exact):
    """The live batch under the settings made: per lane the states after the calls it tracked in,
    its rows before the calls that accepted its later frames, and the window the device's table
    held for each of those frames after that call (FOLLOW)."""
    env, torch, st = pool.env, pool.env.torch, pool.states
    sched = SCHED[pacing]
    lanes, _, x0s = pool.streams(window, input == "u16")
    st.copy_(torch.from_numpy(np.stack([env.start(x) for x in x0s])))
    torch.cuda.synchronize()
    took = [0, 0]
    tracked, rows, tables = [[], []], [[], []], [[], []]

    def frames(step):
        if step is None:
            return None
        fr = [None, None]
        for b in sorted(step):
            fr[b] = lanes[b][took[b]].copy()
            took[b] += 1
        return fr

    env.ctx.refine_exact = exact
    try:
        env.ctx.batch_pipeline_begin(frames(sched[0]), input=input, unit_mm=float(UNIT))
        for k in range(len(sched) - 1):
            prev = st.cpu().numpy().copy()
            for b in (sched[k + 1] or ()):
                rows[b].append(prev[b])  # FOLLOW: the pose the accepted frame's window comes from
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), frames(sched[k + 1]))
            env.sync()
            now = st.cpu().numpy().copy()
            if window == "follow":
                # the table of the parity this call prepared into holds the accepted frames' windows
                tab = env.ctx.batch_windows_readback((k + 1) & 1, 2)
                for b in (sched[k + 1] or ()):
                    tables[b].append(tab[b])
            for b in range(2):
                if b in sched[k]:
                    tracked[b].append(now[b])
                else:  # idle: bit for bit what it was
                    assert np.array_equal(now[b].view(np.uint64), prev[b].view(np.uint64)), (b, k)
    finally:
        env.sync()
        env.ctx.refine_exact = False
    assert took == [NF, NF] and [len(t) for t in tracked] == [NF, NF]
    return tracked, rows, tables


@pytest.mark.parametrize("input,window,pacing,hands,form,refine", CASES)
def test_live_batch(pool, input, window, pacing, hands, form, refine):
    env = pool.env
    exact = refine == "exact"
    wpp = env.ctx.batch_wave_wpp(P, 2)
    yards = pool.yard(hands, form, wpp)
    _, floats, x0s = pool.streams(window)
    init = [y.rule(x) for y, x in zip(yards, x0s)]
    try:
        if hands == "lane":
            env.ctx.set_batch_hands([y.hand for y in yards])
        if window != "off":
            env.ctx.set_batch_window(window, init, MXY, MZ)
        env.ctx.set_batch_form(form)
        env.ctx.set_batch_pacing(pacing)
        tracked, rows, tables = run_batch(pool, input, window, pacing, exact)
    finally:
        env.sync()
        env.ctx.set_batch_pacing("lockstep")
        env.ctx.set_batch_form("auto")
        env.ctx.set_batch_window("off")
        env.ctx.set_batch_hands(None)
    for b, y in enumerate(yards):
        if window == "off":
            want = y.single((b, exact), floats[b], exact)
        else:
            wins = [init[b]] + [init[b] if window == "fixed" else y.rule(r) for r in rows[b]]
            if window == "follow":
                assert tables[b] == wins[1:], b
            want = pool.check_windows(y, b, exact, wins, tracked[b])
        for f in range(NF):
            assert np.array_equal(tracked[b][f], want[f]), (b, f)
    assert np.isfinite(np.array(tracked)).all()
    assert not np.array_equal(tracked[0], tracked[1])


@pytest.mark.parametrize("window,hands,form,refine", RAW_CASES)
def test_raw_batch(pool, window, hands, form, refine):
    """The raw batch's combinations that no other test runs (RAW_COVERED lists the others): the
    streams resident on the device, one chunk of two frames and a tail of one; lane b's history
    row f against the single pipelined loop's state after frame f."""
    env, torch = pool.env, pool.env.torch
    exact = refine == "exact"
    wpp = env.ctx.batch_wave_wpp(P, 2)
    yards = pool.yard(hands, form, wpp)
    _, floats, x0s = pool.streams(window)
    init = [y.rule(x) for y, x in zip(yards, x0s)]
    raws = pool.raw if window == "off" else [pool.raw2, pool.raw2]
    st, hist = pool.states, pool.hist
    st.copy_(torch.from_numpy(np.stack([env.start(x) for x in x0s])))
    hist.fill_(np.nan)
    torch.cuda.synchronize()
    tables = None
    try:
        if hands == "lane":
            env.ctx.set_batch_hands([y.hand for y in yards])
        if window != "off":
            env.ctx.set_batch_window(window, init, MXY, MZ)
        env.ctx.set_batch_form(form)
        env.ctx.refine_exact = exact
        env.ctx.track_raw_batch(P, 1, st.data_ptr(), [r.data_ptr() for r in raws], NF,
                                frames_per_graph=2, d_hist_ptr=hist.data_ptr())
        env.sync()
        if window == "follow":
            tables = [env.ctx.batch_windows_readback(p, 2) for p in (0, 1)]
    finally:
        env.sync()
        env.ctx.refine_exact = False
        env.ctx.set_batch_form("auto")
        env.ctx.set_batch_window("off")
        env.ctx.set_batch_hands(None)
    got, last = hist.cpu().numpy(), st.cpu().numpy()
    for b, y in enumerate(yards):
        if window == "off":
            want = y.single((b, exact), floats[b], exact)
        else:
            # frame 0 through init[b]; FOLLOW: frame 1 by the pose rule on x0, frame g on the
            # lane's state after frame g - 2
            wins = [init[b]] + [init[b] if window == "fixed" else y.rule(x0s[b] if g == 1 else got[b, g - 2])
                                for g in range(1, NF)]
            if window == "follow":  # frame g was prepared into parity g & 1
                assert tables[(NF - 1) & 1][b] == wins[NF - 1], b
                assert tables[(NF - 2) & 1][b] == wins[NF - 2], b
            want = pool.check_windows(y, b, exact, wins, got[b])
        for f in range(NF):
            assert np.array_equal(got[b, f], want[f]), (b, f)
        assert np.array_equal(last[b], want[NF - 1]), b
    assert np.isfinite(got).all()


@pytest.mark.parametrize("hands,form,refine", PREPARED_CASES)
def test_prepared_batch(pool, hands, form, refine):
    """The prepared batch's combinations that no other test runs (PREPARED_COVERED lists the
    others): the two streams in stored slots, one chunk of two frames and a tail of one; lane b's
    history and final state against hpe_track_sequence_dev of its slots alone."""
    env, torch = pool.env, pool.env.torch
    exact = refine == "exact"
    wpp = env.ctx.batch_wave_wpp(P, 2)
    yards = pool.yard(hands, form, wpp)
    for e in [env] + yards:
        e.store(pool.f)
    st, hist = pool.states, pool.hist
    st.copy_(torch.from_numpy(np.stack([env.start(), env.start()])))
    hist.fill_(np.nan)
    torch.cuda.synchronize()
    try:
        if hands == "lane":
            env.ctx.set_batch_hands([y.hand for y in yards])
        env.ctx.set_batch_form(form)
        env.ctx.refine_exact = exact
        env.ctx.track_batch(P, 1, st.data_ptr(), list(SLOT0), NF, 2, hist.data_ptr())
        env.sync()
    finally:
        env.sync()
        env.ctx.refine_exact = False
        env.ctx.set_batch_form("auto")
        env.ctx.set_batch_hands(None)
    got, last = hist.cpu().numpy(), st.cpu().numpy()
    for b, y in enumerate(yards):
        want, final = y.sequence(SLOT0[b], exact)
        assert np.array_equal(got[b], want), b
        assert np.array_equal(last[b], final), b
    assert np.isfinite(got).all()
    assert not np.array_equal(got[0], got[1])
