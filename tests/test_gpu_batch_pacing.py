"""Lane pacing (hpe_set_batch_pacing(HPE_PACING_FREE)): the lanes of a live batch skip calls, join
late and pause.

The yardstick is the single pipelined loop, never the batch: with F0 .. Fm-1 the frames a lane was
given, in order, whatever calls they arrived in, the lane's state after the call that tracks Fi is
state i of hpe_pipeline_begin(F0) + hpe_track_pipelined(..., Fi+1) on a context of the same form,
refine form and hand -- np.array_equal, after EVERY call, on a synchronised stream.  A lane that
does not track in a call must keep its 27 doubles bit for bit: the uint64 views are compared, so
the NaN sentinel in the row of a lane that has not joined yet is checked too.

A schedule is a list of steps: step 0 is the set of lanes given a frame at the begin, step k >= 1
the set given one in the next-frame array of call k - 1, and None the null array that ends the
batch.  A lane tracks in call k iff it was given a frame at step k.

Shapes of test_gpu_batch_live.py: P = 64, maxiter 7 (G = 6), at most 7 synthetic frames per stream.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF = 64, 7, 7
FOCAL, MXY, MZ = 241.42, 1.0, 2.0

# three lanes: lane 0 every step but step 3 (it idles at call 3 while lanes 1 and 2 track; four
# more calls follow, so the refill wait runs on the frame number that idle call published); lane 1
# every second step; lane 2 empty at the begin, joins at step 2, pauses at step 4
GAPS = [{0}, {0, 1}, {0, 2}, {1, 2}, {0}, {0, 1, 2}, {0, 2}, {0, 1}, None]
SHORT = [{0, 1}, {0}, {1, 2}, {0, 2}, {0, 1}, None]


class Env:
    """One context (optionally created with a scaled hand, or under HPE_PSO_FORM / HPE_PSO_WPP):
    the single loop -- the yardstick -- and the free-paced batch."""

    def __init__(self, hand=None, form=None, wpp=None):
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
            self.hand = hpe.scaled_hand(*hand) if hand else hpe.reference_hand(device=0)
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
        self._single = {}  # computed once, shared, never changed
        self.synth = synth
        self.sync()

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def captures(self):
        return self.ctx.graph_captures()

    def evals(self):
        v = C.c_uint64(0)
        self.ctx.check(self.lib.hpe_refine_eval_count(self.ctx.h, C.byref(v), 1))
        return v.value

    def start(self, x0=None):
        x = np.zeros(27)
        x[:26] = self.x0 if x0 is None else np.asarray(x0)[:26]
        return x

    def rule(self, theta):
        S = self.hand.build_hand_model(np.asarray(theta, dtype=np.float64)[:26])
        return self.window.from_spheres(S, self.radii, FOCAL, MXY, MZ)

    def loop(self, frames, refine, row=None):
        """The single pipelined loop over `frames` from state row `row` (default: x0): the state
        after every frame."""
        self.st1.copy_(self.torch.from_numpy(self.start() if row is None else np.asarray(row)))
        self.torch.cuda.synchronize()
        out = []
        n = len(frames)
        self.ctx.pipeline_begin(frames[0])
        for f in range(n):
            self.ctx.track_pipelined(P, refine, self.st1.data_ptr(), frames[f + 1] if f + 1 < n else None)
            self.sync()
            out.append(self.st1.cpu().numpy().copy())
        return np.array(out)

    def single(self, key, frames, refine):
        key = (key, len(frames), refine, self.ctx.refine_exact)
        if key not in self._single:
            self._single[key] = self.loop(frames, refine)
        return self._single[key]

    def batch_states(self, B):
        if B not in self.states:
            self.states[B] = self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0")
        return self.states[B]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(env, lanes, sched, refine, st=None, join_row_at_accept=False, before_call=None,
        windows=None):
    """The free-paced batch over the lanes' frame lists under `sched`.  Lanes not given a frame at
    the begin start with a NaN row, which the test replaces by x0 only just before the call that
    tracks the lane's first frame (join_row_at_accept: before the call that accepts it -- FOLLOW
    reads the pose for that frame's window).  before_call(k, st): runs before call k, the stream
    synchronised.  windows: a dict that receives, per call, both parities' window tables before
    and after it.  Returns a dict: `after` (states after every call, calls x B x 27), `before`
    (before every call), `tracked` (per lane, the calls it tracked in), `given` (per lane, the
    steps it was given a frame at), `rows` (per lane, the state rows recorded before the call of
    each step >= 1 it was given a frame at)."""
    torch = env.torch
    B = len(lanes)
    st = env.batch_states(B) if st is None else st
    x = np.stack([env.start() if b in sched[0] else np.full(27, np.nan) for b in range(B)])
    st.copy_(torch.from_numpy(x))
    torch.cuda.synchronize()
    took = [0] * B  # frames taken from each lane's list

    def frames(step):
        if step is None:
            return None
        fr = [None] * B
        for b in sorted(step):
            fr[b] = lanes[b][took[b]].copy()
            took[b] += 1
        return fr

    def mask(step):
        return sum(1 << b for b in step)

    res = dict(after=[], before=[], tracked=[[] for _ in range(B)], given=[[] for _ in range(B)],
               rows=[[] for _ in range(B)])
    joined = set(sched[0])
    for b in sched[0]:
        res["given"][b].append(0)
    env.ctx.set_batch_pacing("free")
    try:
        env.ctx.batch_pipeline_begin(frames(sched[0]))
        assert env.ctx.batch_pending() == mask(sched[0])
        for k in range(len(sched) - 1):
            pending, nxt = sched[k], sched[k + 1]
            # a joining lane's row: written as late as the contract allows
            for b in range(B):
                if b in joined:
                    continue
                if (b in pending) or (join_row_at_accept and nxt is not None and b in nxt):
                    st[b].copy_(torch.from_numpy(env.start()))
                    joined.add(b)
            torch.cuda.synchronize()
            if before_call:
                before_call(k, st)
                torch.cuda.synchronize()
            prev = st.cpu().numpy().copy()
            res["before"].append(prev)
            if windows is not None:
                windows.setdefault("before", []).append(
                    [env.ctx.batch_windows_readback(p, B) for p in (0, 1)])
            for b in (nxt or ()):
                res["given"][b].append(k + 1)
                res["rows"][b].append(prev[b])
            env.ctx.track_batch_pipelined(P, refine, st.data_ptr(), frames(nxt))
            env.sync()
            now = st.cpu().numpy().copy()
            res["after"].append(now)
            if windows is not None:
                windows.setdefault("after", []).append(
                    [env.ctx.batch_windows_readback(p, B) for p in (0, 1)])
            for b in range(B):
                if b in pending:
                    res["tracked"][b].append(k)
                else:  # idle: bit for bit what it was, NaN sentinel included
                    assert np.array_equal(bits(now[b]), bits(prev[b])), ("idle lane changed", b, k)
            if nxt is not None:
                assert env.ctx.batch_pending() == mask(nxt), k
        m = C.c_uint32(7)
        assert env.lib.hpe_batch_pending(env.ctx.h, C.byref(m)) == env._lib.HPE_E_STATE
        assert m.value == 7
    finally:
        env.sync()
        try:
            env.ctx.set_batch_pacing("lockstep")
        except env.hpe.HpeError:
            pass  # a batch a failed assertion left alive keeps its pacing
    res["after"] = np.array(res["after"])
    return res


def check(env, res, b, want):
    """Lane b's states after the calls it tracked in against the yardstick's states, in order."""
    calls = res["tracked"][b]
    assert len(calls) == len(want), (b, calls)
    for i, k in enumerate(calls):
        assert np.array_equal(res["after"][k, b], want[i]), (b, i, k)


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.streams = [[np.ascontiguousarray(e.ctx.render_depth(th), dtype=np.float32)
                  for th in e.synth.trajectory(NF, s)] for s in range(3)]
    yield e
    e.ctx.close()


def check_streams(env, names, sched, refine, **kw):
    res = run(env, [env.streams[s] for s in names], sched, refine, **kw)
    for b, s in enumerate(names):
        n = len(res["given"][b])
        check(env, res, b, env.single(s, env.streams[s][:n], refine))
    return res


@pytest.mark.parametrize("refine", [1, 0])
def test_full_masks(env, refine):
    """FREE with every lane given every frame: the single loops, as in lockstep."""
    res = check_streams(env, [0, 1, 2], [{0, 1, 2}] * 6 + [None], refine)
    assert np.isfinite(res["after"]).all()
    assert all(len(t) == 6 for t in res["tracked"])


@pytest.mark.parametrize("refine", [1, 0])
def test_gaps(env, refine):
    res = check_streams(env, [0, 1, 2], GAPS, refine)
    assert res["tracked"][0] == [0, 1, 2, 4, 5, 6, 7]  # idle at call 3 while 1 and 2 track
    assert res["tracked"][1] == [1, 3, 5, 7] and res["tracked"][2] == [2, 3, 5, 6]
    assert np.isnan(res["after"][0, 2]).all() and np.isnan(res["after"][1, 2]).all()
    assert np.isfinite(res["after"][2:]).all()


def test_prepare_only_and_track_only_calls(env):
    """Call 0 has an all-null array (track-only), call 1 no pending lane (prepare-only); the
    batch goes on."""
    res = check_streams(env, [1, 2], [{0, 1}, set(), {0, 1}, {0}, {1}, None], 1)
    assert res["tracked"] == [[0, 2, 3], [0, 2, 4]]


def test_sixteen_lanes(env):
    """Lane 0 idles at call 1, lane 15 at call 2 (the table's first and last lane); lane 15 is
    stream 2, the rest stream 0."""
    M = env._lib.BATCH_MAX
    every = set(range(M))
    res = check_streams(env, [0] * (M - 1) + [2], [every, every - {0}, every - {15}, every, None], 1)
    assert res["tracked"][0] == [0, 2, 3] and res["tracked"][15] == [0, 1, 3]
    assert res["tracked"][7] == [0, 1, 2, 3]


@pytest.mark.parametrize("wpp", [1, 2])
def test_wave_form(env, wpp):
    """The batch in the wave form against the single loop in the wave form, both on a context
    created under HPE_PSO_FORM=wave and HPE_PSO_WPP=wpp (the batch's waves per particle are then
    that value)."""
    w = Env(form="wave", wpp=wpp)
    try:
        w.streams = env.streams
        assert w.ctx.batch_wave_wpp(P, 3) == wpp
        w.ctx.set_batch_form("wave")
        check_streams(w, [0, 1, 2], SHORT, 1)
        w.ctx.set_batch_form("auto")
    finally:
        w.ctx.close()


@pytest.mark.parametrize("exact", [False, True])
def test_both_refine_forms(env, exact):
    was = env.ctx.refine_exact
    env.ctx.refine_exact = exact
    try:
        check_streams(env, [0, 1, 2], SHORT, 1)
    finally:
        env.ctx.refine_exact = was


@pytest.mark.parametrize("mode", ["follow", "fixed"])
def test_windows_with_lane_hands_and_gaps(env, mode):
    """Lanes 0 and 2 under the reference hand, lane 1 under a smaller one.  The yardstick is the
    single loop, on a context created with the lane's hand, over frames masked on the host
    (hpe/window.py): a frame given at the begin by init[b], a later one under FOLLOW by the pose
    rule on the row recorded before the call that accepted it, under FIXED by init[b].  The
    window of a lane that accepts no frame in a call stays as it was, in both parities."""
    small = Env(hand=(0.9, 0.85))
    try:
        yards = [env, small, env]
        env.ctx.set_batch_hands([y.hand for y in yards])
        init = [env.ctx.lane_window_from_pose(b, env.x0, FOCAL, MXY, MZ) for b in range(3)]
        assert init[1] == small.rule(env.x0) and init[0] == env.rule(env.x0) and init[1] != init[0]
        env.ctx.set_batch_window(mode, init, MXY, MZ)
        wins = {}
        names = [0, 1, 2]
        res = run(env, [env.streams[s] for s in names], SHORT, 1, join_row_at_accept=True,
                  windows=wins)
    finally:
        env.sync()
        env.ctx.set_batch_window("off")
        env.ctx.set_batch_hands(None)
    try:
        for b, s in enumerate(names):
            masked, rows = [], list(res["rows"][b])
            for i, step in enumerate(res["given"][b]):
                w = init[b] if step == 0 or mode == "fixed" else yards[b].rule(rows.pop(0))
                if mode == "follow" and step > 0:
                    # the table of the parity that call prepared into holds this window
                    assert wins["after"][step - 1][step & 1][b] == w, (b, step)
                    assert not env.window.is_whole(w)
                masked.append(env.window.apply(env.streams[s][i], w))
            check(env, res, b, yards[b].loop(masked, 1))
        # a lane that accepts no frame in call k: its windows are unchanged
        for k in range(len(SHORT) - 1):
            for b in range(3):
                if SHORT[k + 1] is None or b not in SHORT[k + 1]:
                    for p in (0, 1):
                        assert wins["after"][k][p][b] == wins["before"][k][p][b], (k, p, b)
    finally:
        small.ctx.close()


def test_reinitialisation_of_an_idle_lane(env):
    """Lane 1 pauses at calls 2 and 3; between them the caller rewrites its row.  From its next
    frame on the lane equals the single loop restarted from that row on the frames that follow."""
    sched = [{0, 1}, {0, 1}, {0}, {0}, {0, 1}, {0, 1}, None]
    row = env.start(env.x0 + np.r_[0.0, 0.0, 0.0, 0.4, -0.3, 0.5, np.full(20, 1.5)])
    row[26] = 123.0

    def rewrite(k, st):
        if k == 3:
            st[1].copy_(env.torch.from_numpy(row))

    res = run(env, [env.streams[0], env.streams[1]], sched, 1, before_call=rewrite)
    check(env, res, 0, env.single(0, env.streams[0][:6], 1))
    assert res["tracked"][1] == [0, 1, 4, 5]
    head = env.single(1, env.streams[1][:2], 1)
    tail = env.loop(env.streams[1][2:4], 1, row)
    check(env, res, 1, np.concatenate([head, tail]))
    assert np.array_equal(bits(res["after"][3, 1]), bits(row))
    assert not np.array_equal(tail, env.single(1, env.streams[1][:4], 1)[2:])


def test_graphs(env):
    """The masks are never in a graph's key: a batch with a different mask on every call captures
    at most three graphs, a second batch of that shape with other masks none, and a lockstep batch
    afterwards replays what it captured before.  On a context of its own: the live batch's graph
    cache holds 16 graphs and is emptied when full, and the file's context has captured for many
    shapes by now."""
    own = Env()
    own.streams = env.streams
    try:
        _graphs(own)
    finally:
        own.ctx.close()


def _graphs(env):
    torch = env.torch
    st = torch.zeros((3, 27), dtype=torch.float64, device="cuda:0")  # a key of its own
    lanes = [env.streams[s] for s in (2, 0, 1)]

    def lockstep():
        st.copy_(torch.from_numpy(np.stack([env.start()] * 3)))
        torch.cuda.synchronize()
        env.ctx.batch_pipeline_begin([fr[0] for fr in lanes])
        for f in range(3):
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(),
                                          [fr[f + 1] for fr in lanes] if f < 2 else None)
        env.sync()
        return st.cpu().numpy().copy()

    first = lockstep()
    c0 = env.captures()
    run(env, lanes, GAPS, 1, st=st)
    c1 = env.captures()
    assert 1 <= c1 - c0 <= 3
    run(env, lanes, [{1, 2}, {0}, {0, 1, 2}, set(), {2}, {1}, {0, 2}, {0, 1}, None], 1, st=st)
    assert env.captures() == c1
    again = lockstep()
    assert env.captures() == c1
    assert np.array_equal(first, again)
    for b, s in enumerate((2, 0, 1)):
        assert np.array_equal(again[b], env.single(s, env.streams[s][:3], 1)[2])


def test_eval_count_is_the_sum_over_the_tracked_frames(env):
    env.evals()
    total = 0
    for s, n in ((0, 7), (1, 4), (2, 4)):  # the frames GAPS gives each lane
        env.loop(env.streams[s][:n], 1)
        total += env.evals()
    assert total > 0
    run(env, [env.streams[s] for s in (0, 1, 2)], GAPS, 1)
    assert env.evals() == total


def test_refusals_change_nothing(env):
    _lib, torch, lib, h = env._lib, env.torch, env.lib, env.ctx.h
    st = torch.zeros((2, 27), dtype=torch.float64, device="cuda:0")
    sp = C.c_void_p(st.data_ptr())
    f0, f1 = env.streams[0][0], env.streams[0][1]
    p0, p1 = f0.ctypes.data, f1.ctypes.data

    def err():
        return lib.hpe_last_error(h)

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs) if ptrs is not None else None

    def begin(ptrs):
        return lib.hpe_batch_pipeline_begin(h, len(ptrs), arr(ptrs), 1, 1, FOCAL)

    def track(ptrs, B=2):
        return lib.hpe_track_batch_pipelined(h, P, 1, B, sp, arr(ptrs))

    m = C.c_uint32(0)
    assert lib.hpe_batch_pending(h, C.byref(m)) == _lib.HPE_E_STATE and b"no live batch" in err()
    assert lib.hpe_batch_pending(h, None) == _lib.HPE_E_ARG
    for mode in (2, -1):
        assert lib.hpe_set_batch_pacing(h, mode) == _lib.HPE_E_ARG and b"pacing" in err()
    # LOCKSTEP (the default, and still the mode after the refusals above): today's messages
    assert begin([p0, None]) == _lib.HPE_E_ARG and b"null frame array or lane frame" in err()
    assert begin([p0, p0]) == 0
    assert lib.hpe_batch_pending(h, C.byref(m)) == 0 and m.value == 3
    assert track([p1, None]) == _lib.HPE_E_ARG and b"lanes advance in lockstep" in err()
    # a mode change inside a live batch: refused, and the batch goes on in its own mode
    assert lib.hpe_set_batch_pacing(h, _lib.PACING_FREE) == _lib.HPE_E_STATE and b"live batch" in err()
    assert lib.hpe_set_batch_pacing(h, _lib.PACING_LOCKSTEP) == 0
    assert track([p1, None]) == _lib.HPE_E_ARG and b"lockstep" in err()
    st.copy_(torch.from_numpy(np.stack([env.start()] * 2)))
    torch.cuda.synchronize()
    assert track([p1, p1]) == 0 and track(None) == 0
    env.sync()
    want = env.single(0, env.streams[0][:2], 1)[1]
    assert np.array_equal(st[0].cpu().numpy(), want) and np.array_equal(st[1].cpu().numpy(), want)
    # FREE: an all-null begin is refused and begins nothing
    assert lib.hpe_set_batch_pacing(h, _lib.PACING_FREE) == 0
    try:
        assert begin([None, None]) == _lib.HPE_E_ARG and b"at least one" in err()
        assert begin([p0]) == 0 and track(None, B=1) == 0  # usable: a one-lane batch
        assert lib.hpe_batch_pending(h, C.byref(m)) == _lib.HPE_E_STATE
        assert begin([None, p0]) == 0
        assert lib.hpe_batch_pending(h, C.byref(m)) == 0 and m.value == 2
        assert lib.hpe_set_batch_pacing(h, _lib.PACING_LOCKSTEP) == _lib.HPE_E_STATE
        assert lib.hpe_set_batch_pacing(h, _lib.PACING_FREE) == 0
        st.copy_(torch.from_numpy(np.stack([env.start()] * 2)))
        torch.cuda.synchronize()
        assert track([None, None]) == 0  # the batch goes on in its own mode: lane 1 tracks
        assert lib.hpe_batch_pending(h, C.byref(m)) == 0 and m.value == 0
        assert track(None) == 0
        env.sync()
        got = st.cpu().numpy()
        assert np.array_equal(got[1], env.single(0, env.streams[0][:1], 1)[0])
        assert np.array_equal(got[0], env.start())
    finally:
        env.sync()
        assert lib.hpe_set_batch_pacing(h, _lib.PACING_LOCKSTEP) == 0
    check_streams(env, [0, 1, 2], SHORT, 1)
