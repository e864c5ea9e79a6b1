"""The live batch (hpe_batch_pipeline_begin / hpe_track_batch_pipelined): B raw depth streams fed
one host frame per lane and call, every lane's next frame read from its pinned buffer inside the
lanes' refine launch.

Lane b must equal the single pipelined loop of that stream alone on the same context
(hpe_pipeline_begin, then hpe_track_pipelined per frame), bit for bit: np.array_equal on the
27-double state after EVERY frame (the stream is synchronised and the states copied out per
call).  The single loop is the yardstick, never the batch itself.  Small shapes: P = 64, maxiter 7
(G = 6), at most 7 synthetic frames per lane (hpe.synth.trajectory seeds 0, 1, 2, rendered with
render_depth), one context for the whole file.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF = 64, 7, 7


class Env:
    def __init__(self):
        import hpe
        import torch
        from hpe import _lib, synth
        self.hpe, self.torch, self._lib = hpe, torch, _lib
        self.hand = hpe.reference_hand(device=0)
        self.ctx = self.hand.ctx
        self.lib = self.ctx.lib
        ub, lb, sd = hpe.reference_bounds()
        self.pso = hpe.PSO()
        self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        self.pso._push(self.ctx)
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        # streams by name: three synthetic ones, and stream 0 with an all-zero frame 1
        self.streams = {}
        for s in range(3):
            poses = synth.trajectory(NF, s)
            self.streams[s] = [np.ascontiguousarray(self.ctx.render_depth(th), dtype=np.float32)
                               for th in poses]
        hole = [f.copy() for f in self.streams[0][:4]]
        hole[1][:] = 0.0
        self.streams["hole"] = hole
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.states = {}  # B -> the batch's device states: one buffer per lane count (graph keys)
        self._single = {}  # computed once, shared, never changed
        # before any begin on this context: the refusal test reads this
        st = torch.zeros((1, 27), dtype=torch.float64, device="cuda:0")
        self.rc_before_begin = self.lib.hpe_track_batch_pipelined(
            self.ctx.h, P, 1, 1, C.c_void_p(st.data_ptr()), None)
        self.err_before_begin = self.lib.hpe_last_error(self.ctx.h)
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
        x[:26] = self.x0 if x0 is None else x0
        return x

    def single(self, name, n, refine, x0=None, fresh=False):
        """The yardstick: stream `name` alone through the pipelined loop, the state after every
        frame (n x 27)."""
        key = (name, n, refine, self.ctx.refine_exact, None if x0 is None else tuple(x0))
        if fresh or key not in self._single:
            fr = self.streams[name]
            self.st1.copy_(self.torch.from_numpy(self.start(x0)))
            self.torch.cuda.synchronize()
            out = []
            self.ctx.pipeline_begin(fr[0])
            for f in range(n):
                self.ctx.track_pipelined(P, refine, self.st1.data_ptr(), fr[f + 1] if f + 1 < n else None)
                self.sync()
                out.append(self.st1.cpu().numpy().copy())
            if fresh:
                return np.array(out)
            self._single[key] = np.array(out)
        return self._single[key]

    def batch_states(self, B):
        if B not in self.states:
            self.states[B] = self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0")
        return self.states[B]

    def live(self, names, n, refine, x0s=None, scribble=None, between=None, st=None):
        """The live batch over the named streams, a frame per lane and call: the states after
        every frame (n x B x 27).  scribble: the arrays passed are overwritten with that constant
        as soon as each call is back.  between(f): runs after the call of frame f."""
        B = len(names)
        st = self.batch_states(B) if st is None else st
        x = np.stack([self.start(None if x0s is None else x0s[b]) for b in range(B)])
        st.copy_(self.torch.from_numpy(x))
        self.torch.cuda.synchronize()

        def frames(f):
            return [self.streams[nm][f].copy() for nm in names]

        out = []
        fr = frames(0)
        self.ctx.batch_pipeline_begin(fr)
        if scribble is not None:
            for a in fr:
                a[:] = scribble
        for f in range(n):
            fr = frames(f + 1) if f + 1 < n else None
            self.ctx.track_batch_pipelined(P, refine, st.data_ptr(), fr)
            if scribble is not None and fr is not None:
                for a in fr:
                    a[:] = scribble
            self.sync()
            out.append(st.cpu().numpy().copy())
            if between:
                between(f)
        return np.array(out)

    def check_lanes(self, names, n, refine, x0s=None, equal_nan=(), **kw):
        got = self.live(names, n, refine, x0s, **kw)
        for b, nm in enumerate(names):
            want = self.single(nm, n, refine, None if x0s is None else x0s[b])
            for f in range(n):
                assert np.array_equal(got[f, b], want[f], equal_nan=nm in equal_nan), (b, f)
        return got


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


@pytest.mark.parametrize("refine", [1, 0])
def test_three_lanes_six_frames(env, refine):
    """Frames 0..5: the begin and the calls of frames 1 and 3 fill the pinned buffers of parity
    0, the calls of frames 0, 2 and 4 those of parity 1 -- each refilled twice, behind the host's
    wait -- and the last call has no next frame."""
    got = env.check_lanes([0, 1, 2], 6, refine)
    assert np.isfinite(got).all()
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not np.array_equal(got[:, a], got[:, b])


def test_callers_buffers_are_free_after_return(env):
    """The arrays passed to begin and to every call are overwritten with a constant as soon as
    the call is back: the library tracks its own copies."""
    env.check_lanes([0, 1, 2], 6, 1, scribble=1234.5)


def test_lane_order(env):
    """The same three streams in another lane order: the same per-stream results."""
    a = env.check_lanes([0, 1, 2], 5, 1)
    b = env.check_lanes([2, 0, 1], 5, 1)
    assert np.array_equal(b[:, 0], a[:, 2]) and np.array_equal(b[:, 1], a[:, 0])
    assert np.array_equal(b[:, 2], a[:, 1])


def test_identical_lanes_and_one_stream_from_three_poses(env):
    """Two lanes fed identical frames and x0 give identical rows (beside a third, different one);
    three lanes over one stream with different x0 give three different results, each its own
    yardstick's."""
    got = env.check_lanes([1, 0, 1], 4, 1)
    assert np.array_equal(got[:, 0], got[:, 2])
    assert not np.array_equal(got[:, 0], got[:, 1])
    x1, x2 = env.x0.copy(), env.x0.copy()
    x1[3:6] += (0.4, -0.3, 0.5)
    x1[6:] += 1.5
    x2[3:6] -= (0.3, 0.2, -0.4)
    x2[6:] += 0.7
    got = env.check_lanes([0, 0, 0], 4, 1, x0s=[env.x0, x1, x2])
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not np.array_equal(got[:, a], got[:, b])


def test_one_lane(env):
    env.check_lanes([1], 3, 1)


def test_sixteen_lanes(env):
    """The table's first and last lane in both parities: lane 15 is stream 2, the rest stream 0."""
    names = [0] * (env._lib.BATCH_MAX - 1) + [2]
    got = env.check_lanes(names, 3, 1)
    assert not np.array_equal(got[:, 15], got[:, 0])


def test_graph_reuse(env):
    """One graph per frame, keyed by shape: a 5-frame batch captures at most 3 (parity 0 and
    parity 1 with a next frame, one without), and the same batch again -- the same d_states, new
    host arrays -- captures none and reproduces the results."""
    st = env.torch.zeros((2, 27), dtype=env.torch.float64, device="cuda:0")  # a key of its own
    want = [env.single(nm, 5, 1) for nm in (2, 1)]
    before = env.captures()
    first = env.live([2, 1], 5, 1, st=st)
    mid = env.captures()
    assert 1 <= mid - before <= 3
    again = env.live([2, 1], 5, 1, st=st)
    assert env.captures() == mid
    assert np.array_equal(first, again)
    for b in range(2):
        assert np.array_equal(first[:, b], want[b])


@pytest.mark.parametrize("exact", [False, True])
def test_both_refine_forms(env, exact):
    was = env.ctx.refine_exact
    env.ctx.refine_exact = exact
    try:
        env.check_lanes([0, 1, 2], 4, 1)
    finally:
        env.ctx.refine_exact = was


def test_all_zero_frame_in_one_lane(env):
    """Lane 1's frame 1 is all zero: that lane matches its yardstick NaN for NaN, the other lanes
    bit for bit and finite."""
    got = env.check_lanes([1, "hole", 2], 4, 1, equal_nan=("hole",))
    assert np.isfinite(got[:, 0]).all() and np.isfinite(got[:, 2]).all()
    assert not np.array_equal(got[:, 1], env.single(0, 4, 1), equal_nan=True)


def test_interleaved_with_a_single_pipelined_sequence(env):
    """A single pipelined sequence begun before the batch and advanced between the batch's calls:
    both come out as when run apart."""
    n = 4
    alone = env.single(2, n, 1)
    fr = env.streams[2]
    stp = env.torch.zeros(27, dtype=env.torch.float64, device="cuda:0")
    stp.copy_(env.torch.from_numpy(env.start()))
    env.torch.cuda.synchronize()
    env.ctx.pipeline_begin(fr[0])
    mixed = []

    def advance(f):
        env.ctx.track_pipelined(P, 1, stp.data_ptr(), fr[f + 1] if f + 1 < n else None)
        env.sync()
        mixed.append(stp.cpu().numpy().copy())

    env.check_lanes([0, 1], n, 1, between=advance)
    assert np.array_equal(np.array(mixed), alone)


def test_eval_count_is_the_lanes_sum(env):
    env.evals()
    total = 0
    for nm in (0, 1, 2):
        env.single(nm, 3, 1, fresh=True)
        total += env.evals()
    assert total > 0
    env.live([0, 1, 2], 3, 1)
    assert env.evals() == total


def test_raw_batch_ends_a_live_batch(env):
    """hpe_track_raw_batch_dev prepares into the same lane buffers: it ends a live batch in
    progress (HPE_E_STATE for the next live call), and a new begin works as before."""
    torch, _lib = env.torch, env._lib
    st = env.batch_states(2)
    raw = torch.from_numpy(np.stack(env.streams[0][:2])).to("cuda:0")
    st.copy_(torch.from_numpy(np.stack([env.start(), env.start()])))
    torch.cuda.synchronize()
    env.ctx.batch_pipeline_begin([env.streams[0][0], env.streams[1][0]])
    env.ctx.track_raw_batch(P, 1, st.data_ptr(), [raw.data_ptr(), raw.data_ptr()], 2)
    env.sync()
    rc = env.lib.hpe_track_batch_pipelined(env.ctx.h, P, 1, 2, C.c_void_p(st.data_ptr()), None)
    assert rc == _lib.HPE_E_STATE and b"batch" in env.lib.hpe_last_error(env.ctx.h)
    env.check_lanes([0, 1], 3, 1)


def test_refusals_leave_the_context_usable(env, monkeypatch):
    _lib, torch = env._lib, env.torch
    M = _lib.BATCH_MAX
    st = torch.zeros((M + 1, 27), dtype=torch.float64, device="cuda:0")
    sp = C.c_void_p(st.data_ptr())
    f0 = env.streams[0][0]
    p0 = f0.ctypes.data

    def err():
        return env.lib.hpe_last_error(env.ctx.h)

    def arr(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs) if ptrs is not None else None

    def begin(B, ptrs, downsample=1, focal=241.42):
        return env.lib.hpe_batch_pipeline_begin(env.ctx.h, B, arr(ptrs), 1, downsample, focal)

    def track(B, ptrs, num_p=P, states=sp):
        return env.lib.hpe_track_batch_pipelined(env.ctx.h, num_p, 1, B, states, arr(ptrs))

    # no begin yet on this context (taken when the context was made)
    assert env.rc_before_begin == _lib.HPE_E_STATE and b"hpe_batch_pipeline_begin" in env.err_before_begin
    # hpe_batch_pipeline_begin: every refusal returns its code and sets the message
    assert begin(0, [p0]) == _lib.HPE_E_ARG and b"lanes" in err()
    assert begin(M + 1, [p0] * (M + 1)) == _lib.HPE_E_ARG and b"lanes" in err()
    assert begin(1, None) == _lib.HPE_E_ARG and b"null" in err()
    assert begin(2, [p0, None]) == _lib.HPE_E_ARG and b"null" in err()
    assert begin(1, [p0], focal=0.0) == _lib.HPE_E_ARG and b"focal" in err()
    assert begin(1, [p0], focal=-1.0) == _lib.HPE_E_ARG and b"focal" in err()
    assert begin(1, [p0], downsample=0) == _lib.HPE_E_ARG and b"downsample" in err()
    with monkeypatch.context() as m:
        m.setenv("HPE_PIPE_UPLOAD", "1")
        assert begin(1, [p0]) == _lib.HPE_E_STATE and b"HPE_PIPE_UPLOAD" in err()
    # hpe_track_batch_pipelined, a batch of two lanes in progress
    assert begin(2, [p0, p0]) == 0
    assert track(0, [p0]) == _lib.HPE_E_ARG and b"lanes" in err()
    assert track(M + 1, [p0] * (M + 1)) == _lib.HPE_E_ARG and b"lanes" in err()
    assert track(2, [p0, p0], states=None) == _lib.HPE_E_ARG and b"null" in err()
    assert track(2, [p0, None]) == _lib.HPE_E_ARG and b"lockstep" in err()
    assert track(2, [p0, p0], num_p=1024) == _lib.HPE_E_ARG and b"wave form" in err()
    assert track(3, [p0, p0, p0]) == _lib.HPE_E_STATE and b"began with 2" in err()
    assert track(1, [p0]) == _lib.HPE_E_STATE and b"began with 2" in err()
    script = np.zeros((2, 2, 27))
    script[:, :, 26] = 1e300
    env.ctx.subswarm_init_scripted(script, 0)
    try:  # a live transport
        assert track(2, [p0, p0]) == _lib.HPE_E_STATE and b"transport" in err()
        assert begin(2, [p0, p0]) == _lib.HPE_E_STATE and b"transport" in err()
    finally:
        env.ctx.subswarm_fini()
    ext = torch.zeros(27, dtype=torch.float64, device="cuda:0")
    fn = _lib.EXCHANGE_FN(lambda user, d_ext, g: 0)
    env.ctx.check(env.lib.hpe_set_exchange(env.ctx.h, 2, C.c_void_p(ext.data_ptr()),
                                           C.cast(fn, C.c_void_p), None))
    try:  # hpe_set_exchange
        assert track(2, [p0, p0]) == _lib.HPE_E_STATE and b"exchange" in err()
        assert begin(2, [p0, p0]) == _lib.HPE_E_STATE and b"exchange" in err()
    finally:
        env.ctx.check(env.lib.hpe_set_exchange(env.ctx.h, 0, None, None, None))
    # the refused calls left the batch where it was: its last frame, then the batch has ended
    st.zero_()
    st[:2, :26] = torch.from_numpy(env.x0)
    torch.cuda.synchronize()
    assert track(2, None) == 0
    env.sync()
    assert np.array_equal(st[0].cpu().numpy(), env.single(0, 1, 1)[0])
    assert track(2, None) == _lib.HPE_E_STATE and b"ended" in err()
    assert track(2, [p0, p0]) == _lib.HPE_E_STATE and b"ended" in err()
    env.check_lanes([0, 1, 2], 6, 1)
