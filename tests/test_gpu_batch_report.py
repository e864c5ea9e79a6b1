"""Lane reports (hpe_set_batch_report): every tracked frame of a live batch's lane reported to the
host by the device inside the frame's graph -- the state row, the 21 joints under the lane's hand,
their pixels, n and the health flags -- and the same joints for a resident batch's history
(hpe_lane_joints_dev).

Every yardstick is existing code on a separate call, never the report itself: the state is the
lane's row of d_states copied out after hpe_sync and the single pipelined loop of that stream;
the joints are hpe_build_spheres' joints_out at that pose (on a context created with the lane's
hand where lanes have hands); the pixels are hpe.report.project_joints of those joints; n is
hpe_preprocess_depth's n_out of the frame without downsampling (a live batch's tracked cloud is
always downsampled to 250 points, an empty frame's too: the report counts the points found).
All np.array_equal.

Shapes of test_gpu_batch_live.py: P = 64, maxiter 7 (G = 6), at most 7 synthetic frames per lane
(hpe.synth.trajectory seeds 0, 1, 2), one tracking context for the whole file (the lane hands'
yardstick contexts only run hpe_build_spheres).
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF = 64, 7, 7
FOCAL = 241.42


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Env:
    def __init__(self):
        import hpe
        import torch
        from hpe import _lib, report, synth
        self.hpe, self.torch, self._lib, self.report = hpe, torch, _lib, report
        self.hand = hpe.reference_hand(device=0)
        self.ctx = self.hand.ctx
        self.lib = self.ctx.lib
        ub, lb, sd = hpe.reference_bounds()
        self.pso = hpe.PSO()
        self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        self.pso._push(self.ctx)
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        self._hands = {}
        self.streams = {}
        for s in range(3):
            poses = synth.trajectory(NF, s)
            self.streams[s] = [np.ascontiguousarray(self.ctx.render_depth(th), dtype=np.float32)
                               for th in poses]
        hole = [f.copy() for f in self.streams[0][:4]]
        hole[1][:] = 0.0
        self.streams["hole"] = hole
        # the watch test's lanes: one frame held still, and a hand half as large again as the model's
        self.streams["still"] = [self.streams[1][0]] * 4
        big = self.hand_ctx((1.5, 1.5)).ctx
        self.streams["big"] = [np.ascontiguousarray(big.render_depth(th), dtype=np.float32)
                               for th in synth.trajectory(4, 1)]
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.states = {}
        self._single = {}  # computed once, shared, never changed
        self._n = {}
        self.sync()

    def close(self):
        for h in self._hands.values():
            h.ctx.close()
        self.ctx.close()

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def reports_off(self):
        try:
            self.ctx.set_batch_report(0)
        except self.hpe.HpeError:
            pass  # a batch a failed assertion left alive keeps its reports

    def captures(self):
        return self.ctx.graph_captures()

    def evals(self):
        v = C.c_uint64(0)
        self.ctx.check(self.lib.hpe_refine_eval_count(self.ctx.h, C.byref(v), 1))
        return v.value

    def err(self):
        return self.lib.hpe_last_error(self.ctx.h)

    def start(self):
        x = np.zeros(27)
        x[:26] = self.x0
        return x

    def single(self, name, n, refine=1):
        """The yardstick: stream `name` alone through the pipelined loop, the state after every
        frame (n x 27)."""
        key = (name, n, refine)
        if key not in self._single:
            fr = self.streams[name]
            self.st1.copy_(self.torch.from_numpy(self.start()))
            self.torch.cuda.synchronize()
            out = []
            self.ctx.pipeline_begin(fr[0])
            for f in range(n):
                self.ctx.track_pipelined(P, refine, self.st1.data_ptr(), fr[f + 1] if f + 1 < n else None)
                self.sync()
                out.append(self.st1.cpu().numpy().copy())
            self._single[key] = np.array(out)
        return self._single[key]

    def n_of(self, name, f):
        """hpe_preprocess_depth's n_out of frame f of a stream: its points before downsampling."""
        if (name, f) not in self._n:
            self._n[(name, f)] = len(self.hpe.preprocess_depth(self.streams[name][f],
                                                               downsample=False)["cloud"])
        return self._n[(name, f)]

    def hand_ctx(self, scales):
        """A separate context created with a hand: None the reference hand, else scaled_hand."""
        if scales not in self._hands:
            self._hands[scales] = (self.hpe.reference_hand(device=0) if scales is None
                                   else self.hpe.scaled_hand(*scales))
        return self._hands[scales]

    def joints_at(self, state, hand=None):
        """hpe_build_spheres' joints_out at the pose of a state row, on the given hand's context."""
        _, J = (hand or self.hand).build_batch(np.asarray(state, dtype=np.float64)[:26])
        return J[0]

    def batch_states(self, B):
        if B not in self.states:
            self.states[B] = self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0")
        return self.states[B]

    def live(self, names, n, refine=1, between=None, st=None, sync=True):
        """The live batch in lockstep over the named streams: the states after every frame
        (n x B x 27; sync=False: none, and nothing synchronises).  between(f, states_f): after the
        call of frame f."""
        B = len(names)
        st = self.batch_states(B) if st is None else st
        st.copy_(self.torch.from_numpy(np.stack([self.start()] * B)))
        self.torch.cuda.synchronize()
        out = []
        self.ctx.batch_pipeline_begin([self.streams[nm][0].copy() for nm in names])
        for f in range(n):
            fr = [self.streams[nm][f + 1].copy() for nm in names] if f + 1 < n else None
            self.ctx.track_batch_pipelined(P, refine, st.data_ptr(), fr)
            if sync:
                self.sync()
                out.append(st.cpu().numpy().copy())
            if between:
                between(f, out[-1] if sync else None)
        return np.array(out)

    def check_report(self, r, state, hand=None, equal_nan=False):
        """A report against the yardsticks of its state row: the row itself, the joints at that
        pose and the mirror's pixels; F_NAN iff an entry is not finite."""
        assert np.array_equal(r.state, state, equal_nan=equal_nan)
        if not equal_nan:
            assert np.array_equal(bits(r.state), bits(state))
        J = self.joints_at(state, hand)
        assert np.array_equal(r.joints, J, equal_nan=equal_nan)
        assert np.array_equal(r.px, self.report.project_joints(J, FOCAL), equal_nan=True)
        assert np.array_equal(r.px, self.report.project_joints(r.joints, FOCAL), equal_nan=True)
        assert bool(r.flags & self._lib.REPORT_F_NAN) == (not np.isfinite(state).all())
        assert r.state.shape == (27,) and r.joints.shape == (21, 3) and r.px.shape == (21, 2)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


@pytest.fixture
def reports(env):
    """Reports on for one test (depth 4, no watch unless the test sets its own), off after it."""
    env.ctx.set_batch_report(4)
    yield env
    env.sync()
    env.reports_off()


def test_lockstep_two_lanes(reports):
    env, _lib = reports, reports._lib
    names, n = [0, 1], 4
    seen = []

    def after(f, states):
        for b, nm in enumerate(names):
            r = env.ctx.batch_report(b)
            assert (r.seq, r.call, r.lane, r.kind) == (f + 1, f + 1, b, _lib.REPORT_TRACK), (f, b)
            env.check_report(r, states[b])
            assert np.isfinite(r.px).all() and np.isfinite(r.joints).all()
            assert np.array_equal(r.state, env.single(nm, n)[f]), (f, b)
            assert r.n == env.n_of(nm, f) and r.n > 0, (f, b)
            assert r.flags == 0 and r.bad_streak == 0
            # the same report by its number, and through the wait
            for q in (env.ctx.batch_report(b, f + 1), env.ctx.batch_report_wait(b, 0, 0),
                      env.ctx.batch_report_wait(b, f + 1, 1)):
                assert q.seq == r.seq and np.array_equal(q.state, r.state) and np.array_equal(q.px, r.px)
            seen.append(r)
        assert env.ctx.batch_lost() == 0

    env.live(names, n, between=after)
    assert len(seen) == 2 * n
    # joints of different lanes and frames differ: the reports are not one lane's copied around
    # (the streams share their first pose: the lanes are compared at the last frame)
    assert not np.array_equal(seen[-1].joints, seen[-2].joints)
    assert not np.array_equal(seen[0].joints, seen[2].joints)
    # the rings survive the end of the batch
    assert env.ctx.batch_report(0).seq == n and env.ctx.batch_report(1, 1).seq == 1


def test_reports_change_nothing(env):
    env.ctx.set_batch_report(0)
    env.evals()
    off = env.live([0, 1], 4)
    ev_off = env.evals()
    env.ctx.set_batch_report(4, (1e300, 0, 3))
    try:
        on = env.live([0, 1], 4)
    finally:
        env.reports_off()
    assert ev_off > 0 and env.evals() == ev_off
    assert np.array_equal(bits(on), bits(off))


def test_hole_stream(reports):
    """Lane 0's frame 1 is all zero, beside a healthy lane."""
    env, _lib = reports, reports._lib
    names, n = ["hole", 1], 4
    reps = []
    got = env.live(names, n, between=lambda f, s: reps.append([env.ctx.batch_report(b) for b in (0, 1)]))
    for f in range(n):
        hole, ok = reps[f]
        assert (hole.seq, ok.seq) == (f + 1, f + 1)
        env.check_report(hole, got[f, 0], equal_nan=True)
        env.check_report(ok, got[f, 1])
        assert ok.flags == 0 and ok.bad_streak == 0 and ok.n == env.n_of(1, f)
        assert np.array_equal(got[f, 0], env.single("hole", n)[f], equal_nan=True)
        assert bool(hole.flags & _lib.REPORT_F_EMPTY) == (f == 1)
        # the default watch {+inf, 0, 0}: only a NaN cost is suspect, and nothing is ever lost
        assert bool(hole.flags & _lib.REPORT_F_SUSPECT) == bool(np.isnan(got[f, 0, 26]))
        assert not hole.flags & _lib.REPORT_F_LOST
    assert reps[1][0].n == 0 and reps[0][0].n == env.n_of(0, 0) > 250
    assert env.ctx.batch_lost() == 0


def test_watch_and_init_report(env):
    """cost_max strictly between the two lanes' costs, streak 2: the costlier lane is SUSPECT
    from its first report and LOST from its second; after hpe_batch_pipeline_optimise on it an
    INIT report arrives with the streak zeroed."""
    _lib = env._lib
    names = ["still", "big"]
    costs = env.live(names, 3)[:, :, 26]  # the two lanes once, reports off
    hi = int(np.argmax(costs[0]))
    lo = 1 - hi
    cost_max = 0.5 * (costs[:2, lo].max() + costs[:2, hi].min())
    print("costs per frame", costs.tolist(), "cost_max", cost_max)
    # the premise: the threshold separates the lanes in the first two frames
    assert (costs[:2, hi] > cost_max).all() and (costs[:2, lo] < cost_max).all()
    st = env.batch_states(2)
    env.ctx.set_batch_report(4, (cost_max, 0, 2))
    try:
        def after(f, states):
            r_hi, r_lo = env.ctx.batch_report(hi), env.ctx.batch_report(lo)
            if f == 0:
                assert r_hi.flags == _lib.REPORT_F_SUSPECT and r_hi.bad_streak == 1
                assert env.ctx.batch_lost() == 0
            if f == 1:
                assert r_hi.flags == _lib.REPORT_F_SUSPECT | _lib.REPORT_F_LOST and r_hi.bad_streak == 2
                assert env.ctx.batch_lost() == 1 << hi
                # the application's move: re-initialise the lost lane on its prepared frame
                env.ctx.batch_pipeline_optimise(P, st.data_ptr(), lanes=1 << hi)
                ini = env.ctx.batch_report_wait(hi, 0, 5000)
                assert (ini.seq, ini.call, ini.kind, ini.lane) == (3, 2, _lib.REPORT_INIT, hi)
                assert ini.flags == 0 and ini.bad_streak == 0
                assert ini.n == env.n_of(names[hi], 2)  # the frame it holds prepared
                env.sync()
                rows = st.cpu().numpy()
                env.check_report(ini, rows[hi])
                assert not np.array_equal(rows[hi], states[hi])  # the row was rewritten
                assert np.array_equal(bits(rows[lo]), bits(states[lo]))
                assert env.ctx.batch_lost() == 0
                assert env.ctx.batch_report(lo).seq == 2  # no INIT report for the other lane
            if f == 2:  # the streak starts again after the INIT report
                want = not states[hi][26] <= cost_max
                assert (r_hi.seq, r_hi.kind, r_hi.call) == (4, _lib.REPORT_TRACK, 3)
                assert r_hi.bad_streak == (1 if want else 0)
                assert r_hi.flags == (_lib.REPORT_F_SUSPECT if want else 0)
            if f < 2:
                assert r_lo.flags == 0 and r_lo.bad_streak == 0
            env.check_report(r_hi, states[hi])
            env.check_report(r_lo, states[lo])

        env.live(names, 3, between=after)
    finally:
        env.reports_off()


@pytest.mark.parametrize("odd", [0, 15])
def test_sixteen_lanes_with_lane_hands(env, odd):
    scales = [None] * 16
    scales[odd] = (0.9, 0.85)
    hands = [env.hand_ctx(s) for s in scales]
    names = [0] * 15 + [2] if odd == 0 else [2] + [0] * 15
    env.ctx.set_batch_hands(hands)
    env.ctx.set_batch_report(2)
    try:
        got = env.live(names, 2)
        reps = [env.ctx.batch_report(b) for b in range(16)]
    finally:
        env.reports_off()
        env.ctx.set_batch_hands(None)
    for b, r in enumerate(reps):
        assert (r.seq, r.lane, r.flags) == (2, b, 0)
        env.check_report(r, got[1, b], hand=hands[b])
    # the odd hand matters: its lane's joints are not the reference hand's at the same pose
    assert not np.array_equal(reps[odd].joints, env.joints_at(got[1, odd], env.hand_ctx(None)))


def test_free_pacing(env):
    """Three lanes: lane 0 starts empty and idles in the first tracked call, lane 1 skips a
    middle call."""
    _lib, torch = env._lib, env.torch
    sched = [{1, 2}, {0, 1, 2}, {0, 2}, {0, 1, 2}, None]  # step k: the lanes given a frame
    B = 3
    st = env.batch_states(B)
    x = np.stack([env.start() if b in sched[0] else np.full(27, np.nan) for b in range(B)])
    st.copy_(torch.from_numpy(x))
    torch.cuda.synchronize()
    took = [0] * B

    def frames(step):
        if step is None:
            return None
        fr = [None] * B
        for b in sorted(step):
            fr[b] = env.streams[b][took[b]].copy()
            took[b] += 1
        return fr

    def raw(b):
        return bytes(env.ctx.batch_report(b, raw=True))

    env.ctx.set_batch_pacing("free")
    env.ctx.set_batch_report(4)
    try:
        env.ctx.batch_pipeline_begin(frames(sched[0]))
        tracked = [0] * B
        for k in range(len(sched) - 1):
            pending, nxt = sched[k], sched[k + 1]
            if k == 1:  # lane 0 joins: its row just before the call that tracks its first frame
                st[0].copy_(torch.from_numpy(env.start()))
                torch.cuda.synchronize()
            before = [raw(b) for b in range(B)]
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), frames(nxt))
            env.sync()
            rows = st.cpu().numpy()
            for b in range(B):
                if b not in pending:  # idle: its newest report is byte for byte what it was
                    assert raw(b) == before[b], (k, b)
                    continue
                tracked[b] += 1
                r = env.ctx.batch_report(b)
                assert (r.seq, r.call, r.kind, r.lane) == (tracked[b], k + 1, _lib.REPORT_TRACK, b)
                env.check_report(r, rows[b])
                assert r.n == env.n_of(b, tracked[b] - 1) and r.flags == 0
            assert env.ctx.batch_report(0).seq == tracked[0]
        assert tracked == [3, 3, 4]
        for b in range(B):  # each lane's reports: the single loop over the frames it was given
            want = env.single(b, tracked[b])
            for q in range(max(1, tracked[b] - 3), tracked[b] + 1):
                assert np.array_equal(env.ctx.batch_report(b, q).state, want[q - 1]), (b, q)
    finally:
        env.sync()
        env.reports_off()
        try:
            env.ctx.set_batch_pacing("lockstep")
        except env.hpe.HpeError:
            pass  # a batch a failed assertion left alive keeps its pacing


def test_wave_form(env):
    env.ctx.set_batch_form("wave")
    env.ctx.set_batch_report(4)
    try:
        reps = []
        got = env.live([1, 2], 3, between=lambda f, s: reps.append([env.ctx.batch_report(b) for b in (0, 1)]))
    finally:
        env.sync()
        env.reports_off()
        env.ctx.set_batch_form("auto")
    for f in range(3):
        for b in range(2):
            assert (reps[f][b].seq, reps[f][b].call, reps[f][b].flags) == (f + 1, f + 1, 0)
            env.check_report(reps[f][b], got[f, b])


def test_ring_of_two(env):
    """Depth 2, five calls and no read in between."""
    _lib = env._lib
    env.ctx.set_batch_report(2)
    try:
        env.live([0, 1], 5, sync=False)
        env.sync()
        rows = env.batch_states(2).cpu().numpy()
        for b, nm in enumerate([0, 1]):
            r = env.ctx.batch_report(b)
            assert (r.seq, r.call) == (5, 5)
            env.check_report(r, rows[b])
            r4 = env.ctx.batch_report(b, 4)
            assert r4.seq == 4 and np.array_equal(r4.state, env.single(nm, 5)[3])
            out = _lib.LaneReport()
            for seq in (3, 6):
                assert env.lib.hpe_batch_report(env.ctx.h, b, seq, C.byref(out)) == _lib.HPE_E_STATE
                assert b"not in the ring" in env.err()
                assert env.lib.hpe_batch_report_wait(env.ctx.h, b, seq, 1, C.byref(out)) == _lib.HPE_E_STATE
    finally:
        env.reports_off()


def test_no_synchronisation(reports):
    """Nothing synchronises between the begin and the last wait: the wait alone delivers the
    report, which is the d_states row a later hpe_sync shows."""
    env = reports
    got = []
    env.live([2, 1], 2, sync=False,
             between=lambda f, s: got.append([env.ctx.batch_report_wait(b, 0, 2000) for b in (0, 1)]))
    last = [env.ctx.batch_report(b) for b in (0, 1)]  # complete by now: no wait, no stream
    env.sync()
    rows = env.batch_states(2).cpu().numpy()
    for b, nm in enumerate([2, 1]):
        assert got[0][b].seq == 1 and got[1][b].seq == 2 and last[b].seq == 2
        assert np.array_equal(bits(got[1][b].state), bits(rows[b]))
        assert np.array_equal(bits(last[b].state), bits(rows[b]))
        env.check_report(got[1][b], rows[b])
        env.check_report(got[0][b], env.single(nm, 2)[0])


def _report_arrays(env, names, n):
    """Every report of a lockstep batch, as arrays (n x B x ...)."""
    reps = []
    env.live(names, n, between=lambda f, s: reps.append([env.ctx.batch_report(b) for b in range(len(names))]))
    return dict(head=np.array([[(r.seq, r.call, r.lane, r.kind, r.n, r.flags, r.bad_streak) for r in fr]
                               for fr in reps]),
                state=np.array([[r.state for r in fr] for fr in reps]),
                joints=np.array([[r.joints for r in fr] for fr in reps]),
                px=np.array([[r.px for r in fr] for fr in reps]))


def test_graphs(env, tmp_path):
    torch = env.torch
    st = torch.zeros((2, 27), dtype=torch.float64, device="cuda:0")  # a key of its own
    env.ctx.set_batch_report(4)
    try:
        before = env.captures()
        first = env.live([2, 1], 5, st=st)
        mid = env.captures()
        assert 1 <= mid - before <= 3
        again = env.live([2, 1], 5, st=st)
        assert env.captures() == mid
        env.ctx.set_batch_report(0)
        off = env.live([2, 1], 5, st=st)
        mid2 = env.captures()
        assert mid2 - mid <= 3  # the graphs without the report launch: other keys
        env.ctx.set_batch_report(4)
        on = env.live([2, 1], 5, st=st)
        env.ctx.set_batch_report(0)
        off2 = env.live([2, 1], 5, st=st)
        assert env.captures() == mid2  # off and on again: replayed, nothing captured
        for a in (again, off, on, off2):
            assert np.array_equal(bits(a), bits(first))
        env.ctx.set_batch_report(4)
        mine = _report_arrays(env, [0, 1], 4)
    finally:
        env.reports_off()
    # direct launches (HPE_NO_GRAPH=1, read at hpe_create): a fresh process, the same reports
    out = tmp_path / "reports.npz"
    sub = subprocess.run([sys.executable, __file__, str(out)], env=dict(os.environ, HPE_NO_GRAPH="1"),
                         capture_output=True, text=True, timeout=120)
    assert sub.returncode == 0, sub.stdout + sub.stderr
    theirs = np.load(out)
    for k, v in mine.items():
        assert np.array_equal(theirs[k], v, equal_nan=True), k
    assert int(theirs["captures"]) == 0


def test_lane_joints_of_a_raw_batch(env):
    torch = env.torch
    B, n = 3, 4
    scales = [None, (0.9, 0.85), (1.1, 1.2)]
    hands = [env.hand_ctx(s) for s in scales]
    raws = [torch.from_numpy(np.stack(env.streams[b][:n])).to("cuda:0") for b in range(B)]
    st = env.batch_states(B)
    st.copy_(torch.from_numpy(np.stack([env.start()] * B)))
    hist = torch.zeros((B, n, 27), dtype=torch.float64, device="cuda:0")
    J = torch.full((B, n, 21, 3), -7.0, dtype=torch.float64, device="cuda:0")
    px = torch.full((B, n, 21, 2), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    env.ctx.set_batch_hands(hands)
    try:
        env.ctx.track_raw_batch(P, 1, st.data_ptr(), [r.data_ptr() for r in raws], n,
                                d_hist_ptr=hist.data_ptr())
        env.ctx.lane_joints(B, n, hist.data_ptr(), J.data_ptr(), px.data_ptr(), FOCAL)
        env.sync()
        h, j, p = hist.cpu().numpy(), J.cpu().numpy(), px.cpu().numpy()
        assert np.isfinite(h).all()
        for b in range(B):
            _, want = hands[b].build_batch(h[b, :, :26])
            assert np.array_equal(j[b], want), b
            assert np.array_equal(p[b], env.report.project_joints(want, FOCAL)), b
        assert not np.array_equal(j[1], hands[0].build_batch(h[1, :, :26])[1])  # the lane's own hand
        # without pixels; then a NaN row: NaN for that row, the others untouched
        J2 = torch.full_like(J, -7.0)
        torch.cuda.synchronize()
        env.ctx.lane_joints(B, n, hist.data_ptr(), J2.data_ptr(), None)
        env.sync()
        hist[1, 2, :] = float("nan")
        J3, px3 = torch.full_like(J, -7.0), torch.full_like(px, -7.0)
        torch.cuda.synchronize()
        env.ctx.lane_joints(B, n, hist.data_ptr(), J3.data_ptr(), px3.data_ptr(), FOCAL)
        env.sync()
        assert np.array_equal(J2.cpu().numpy(), j)
        j3, p3 = J3.cpu().numpy(), px3.cpu().numpy()
        assert np.isnan(j3[1, 2]).all() and np.isnan(p3[1, 2]).all()
        keep = np.ones((B, n), dtype=bool)
        keep[1, 2] = False
        assert np.array_equal(j3[keep], j[keep]) and np.array_equal(p3[keep], p[keep])
        # refusals
        _lib, lib, h_ = env._lib, env.lib, env.ctx.h
        hp, jp, pp = (C.c_void_p(t.data_ptr()) for t in (hist, J, px))
        for args, word in (((0, n, hp, FOCAL, jp, pp), b"lanes"), ((17, n, hp, FOCAL, jp, pp), b"lanes"),
                           ((B, 0, hp, FOCAL, jp, pp), b"rows"), ((B, n, None, FOCAL, jp, pp), b"null"),
                           ((B, n, hp, FOCAL, None, pp), b"null"), ((B, n, hp, 0.0, jp, pp), b"focal"),
                           ((B, n, hp, -1.0, jp, pp), b"focal")):
            assert lib.hpe_lane_joints_dev(h_, *args) == _lib.HPE_E_ARG and word in env.err(), args
        assert lib.hpe_lane_joints_dev(h_, B, n, hp, 0.0, jp, None) == 0  # no pixels: focal unused
        env.sync()
    finally:
        env.ctx.set_batch_hands(None)


def test_refusals_leave_the_context_as_it_was(env):
    _lib, lib, h = env._lib, env.lib, env.ctx.h
    W = _lib.ReportWatch
    out = _lib.LaneReport()
    env.ctx.set_batch_report(4, (1e300, 0, 2))
    try:
        for depth in (1, 65, -1):
            assert lib.hpe_set_batch_report(h, depth, None) == _lib.HPE_E_ARG and b"depth" in env.err()
        assert lib.hpe_set_batch_report(h, 4, C.byref(W(1.0, 0, -1))) == _lib.HPE_E_ARG and b"streak" in env.err()
        assert lib.hpe_set_batch_report(h, 4, C.byref(W(1.0, -1, 0))) == _lib.HPE_E_ARG and b"n_min" in env.err()

        def mid(f, states):
            if f != 1:
                return
            # a live batch in progress keeps its reports: another depth, another watch, off
            for depth, w in ((8, W(1e300, 0, 2)), (4, W(5.0, 0, 2)), (4, None), (0, None)):
                rc = lib.hpe_set_batch_report(h, depth, C.byref(w) if w else None)
                assert rc == _lib.HPE_E_STATE and b"live batch" in env.err()
            assert lib.hpe_set_batch_report(h, 4, C.byref(W(1e300, 0, 2))) == 0  # the same: no change
            for lane in (-1, 2, 16):
                assert lib.hpe_batch_report(h, lane, 0, C.byref(out)) == _lib.HPE_E_ARG and b"lane" in env.err()
                assert lib.hpe_batch_report_wait(h, lane, 0, 1, C.byref(out)) == _lib.HPE_E_ARG
            assert lib.hpe_batch_report(h, 0, 0, None) == _lib.HPE_E_ARG and b"null" in env.err()
            assert lib.hpe_batch_report_wait(h, 0, 0, 1, None) == _lib.HPE_E_ARG
            assert lib.hpe_batch_lost(h, None) == _lib.HPE_E_ARG
            assert lib.hpe_batch_report_wait(h, 0, 3, 1, C.byref(out)) == _lib.HPE_E_STATE  # not enqueued

        got = env.live([0, 1], 4, between=mid)
        for b, nm in enumerate([0, 1]):  # the batch went on as if nothing had been asked
            assert np.array_equal(got[:, b], env.single(nm, 4))
            r = env.ctx.batch_report(b)
            assert (r.seq, r.call, r.flags) == (4, 4, 0)
            env.check_report(r, got[3, b])
    finally:
        env.reports_off()
    # a batch begun with reports off leaves nothing to read
    env.live([0, 1], 1)
    assert lib.hpe_batch_report(h, 0, 0, C.byref(out)) == _lib.HPE_E_STATE and b"reports" in env.err()
    m = C.c_uint32(5)
    assert lib.hpe_batch_lost(h, C.byref(m)) == _lib.HPE_E_STATE and m.value == 5


if __name__ == "__main__":  # test_graphs' child: the reports of [0, 1] x 4 under the environment
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "hand-pose-estimation_amd"), str(root / "oracle"), str(root / "tests")]
    import torch
    torch.cuda.is_available()  # torch's HIP runtime first, as conftest.py has it
    e = Env()
    e.ctx.set_batch_report(4)
    arrays = _report_arrays(e, [0, 1], 4)
    np.savez(sys.argv[1], captures=e.captures(), **arrays)
    e.ctx.set_batch_report(0)
    e.close()
