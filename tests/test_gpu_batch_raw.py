"""Batched raw tracking (hpe_track_raw_batch_dev): B resident raw sequences in the same launches,
each lane's next frame prepared inside the lanes' refine launch.

Lane b of a batch must equal hpe_track_raw_sequence_dev of that lane alone on the same context,
bit for bit: np.array_equal on the whole n x 27 history and on the final state.  The
single-sequence path is the yardstick, never the batch itself.  Small shapes: P = 64, maxiter 7
(G = 6), at most 7 synthetic frames per lane (hpe.synth.trajectory seeds 0, 1, 2, rendered and
uploaded as raw float mm), one context for the whole file.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF = 64, 7, 7
SLOT0 = (10, 20)           # two prepared sequences for hpe_track_batch_dev (graph reuse test)
SENTINEL = -7.0


class Env:
    def __init__(self):
        import hpe
        import torch
        from hpe import synth
        self.hpe, self.torch = hpe, torch
        self.hand = hpe.reference_hand(device=0)
        self.ctx = self.hand.ctx
        self.lib = self.ctx.lib
        ub, lb, sd = hpe.reference_bounds()
        self.pso = hpe.PSO()
        self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        self.pso._push(self.ctx)
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        self.depth = []
        for s in range(3):
            poses = synth.trajectory(NF, s)
            self.depth.append([np.ascontiguousarray(self.ctx.render_depth(th)) for th in poses])
        self.raw = [self.upload(np.stack(d)) for d in self.depth]
        hole = np.stack(self.depth[0][:3])
        hole[1] = 0.0
        self.raw_hole = self.upload(hole)  # sequence 0 with an all-zero frame 1
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.h1 = torch.empty((NF, 27), dtype=torch.float64, device="cuda:0")
        self.bufs = {}    # (B, n) -> (states, hist): one buffer pair per shape (graph keys)
        self._alone = {}  # computed once, shared, never changed
        self.sync()

    def upload(self, frames):
        return self.torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to("cuda:0")

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def captures(self):
        return self.ctx.graph_captures()

    def evals(self, reset=True):
        v = C.c_uint64(0)
        self.ctx.check(self.lib.hpe_refine_eval_count(self.ctx.h, C.byref(v), 1 if reset else 0))
        return v.value

    def start(self, x0=None):
        x = np.zeros(27)
        x[:26] = self.x0 if x0 is None else x0
        return x

    def alone(self, raw, n, refine, x0=None, fresh=False):
        """track_raw_sequence of one lane alone: (history n x 27, final state)."""
        exact = self.ctx.refine_exact
        key = (raw.data_ptr(), n, refine, exact, None if x0 is None else tuple(x0))
        if fresh or key not in self._alone:
            self.st1.copy_(self.torch.from_numpy(self.start(x0)))
            self.h1.fill_(SENTINEL)
            self.torch.cuda.synchronize()
            self.ctx.track_raw_sequence(P, refine, self.st1.data_ptr(), raw.data_ptr(), n,
                                        frames_per_graph=4, d_hist_ptr=self.h1.data_ptr())
            self.sync()
            r = (self.h1.cpu().numpy()[:n].copy(), self.st1.cpu().numpy().copy())
            if fresh:
                return r
            self._alone[key] = r
        return self._alone[key]

    def batch(self, raws, n, refine, K, x0s=None):
        """track_raw_batch over the lanes' raw buffers: (history B x n x 27, states B x 27)."""
        B = len(raws)
        if (B, n) not in self.bufs:
            self.bufs[(B, n)] = (self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0"),
                                 self.torch.empty((B, n, 27), dtype=self.torch.float64, device="cuda:0"))
        st, hist = self.bufs[(B, n)]
        x = np.stack([self.start(None if x0s is None else x0s[b]) for b in range(B)])
        st.copy_(self.torch.from_numpy(x))
        hist.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        self.ctx.track_raw_batch(P, refine, st.data_ptr(), [r.data_ptr() for r in raws], n,
                                 frames_per_graph=K, d_hist_ptr=hist.data_ptr())
        self.sync()
        return hist.cpu().numpy(), st.cpu().numpy()

    def check_lanes(self, raws, n, refine, K, x0s=None, equal_nan=False):
        hist, st = self.batch(raws, n, refine, K, x0s)
        for b, raw in enumerate(raws):
            ah, a_st = self.alone(raw, n, refine, None if x0s is None else x0s[b])
            assert np.array_equal(hist[b], ah, equal_nan=equal_nan), b
            assert np.array_equal(st[b], a_st, equal_nan=equal_nan), b
        return hist, st


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


@pytest.mark.parametrize("refine", [1, 0])
def test_three_lanes_chunk_and_tail(env, refine):
    """B = 3 distinct lanes, n = 6 in chunks of 4: a full chunk and a 2-frame tail chunk, the
    buffer parity and the cursors crossing a graph boundary."""
    hist, _ = env.check_lanes(env.raw, 6, refine, 4)
    assert not np.array_equal(hist[0], hist[1]) and not np.array_equal(hist[1], hist[2])
    assert not np.array_equal(hist[0], hist[2])
    assert not (hist == SENTINEL).any()


def test_odd_chunk_length(env):
    """n = 7 in chunks of 3: chunks start on both buffer parities (frames 0, 3, 6), with a next
    frame to prepare after their last one and without."""
    hist, _ = env.check_lanes(env.raw, 7, 1, 3)
    assert not (hist == SENTINEL).any()


@pytest.mark.parametrize("exact", [False, True])
def test_both_refine_forms(env, exact):
    was = env.ctx.refine_exact
    env.ctx.refine_exact = exact
    try:
        env.check_lanes(env.raw, 6, 1, 4)
    finally:
        env.ctx.refine_exact = was


def test_one_lane_is_track_raw_sequence(env):
    env.check_lanes([env.raw[1]], 6, 1, 4)


def test_two_lanes_on_the_same_raw_buffer(env):
    """Two hands in one depth stream: the same raw buffer, different x0."""
    x1 = env.x0.copy()
    x1[3:6] += (0.4, -0.3, 0.5)
    x1[6:] += 1.5
    hist, _ = env.check_lanes([env.raw[0], env.raw[0]], 5, 1, 4, x0s=[env.x0, x1])
    assert not np.array_equal(hist[0], hist[1])


def test_full_batch(env):
    from hpe import _lib
    env.check_lanes([env.raw[b % 3] for b in range(_lib.BATCH_MAX)], 2, 1, 1)


def test_graph_reuse_and_the_other_calls(env):
    """Chunk graphs are keyed by shape: the same call over permuted raw pointers, and over
    freshly allocated raw buffers of the same shape, captures nothing.  The call keeps to its
    own buffers: a pipelined sequence it interrupts goes on, and track_raw_sequence and
    track_batch over prepared slots give their earlier bits afterwards."""
    ctx, torch = env.ctx, env.torch
    d = env.depth[0]
    for s in range(2):
        for f in range(3):
            ctx.prepare_frame(SLOT0[s] + f, env.depth[s][f])
    env.sync()
    stb = torch.zeros((2, 27), dtype=torch.float64, device="cuda:0")
    hb = torch.empty((2, 3, 27), dtype=torch.float64, device="cuda:0")
    stp = torch.zeros(27, dtype=torch.float64, device="cuda:0")

    def prepared_batch():
        stb.copy_(torch.from_numpy(np.stack([env.start(), env.start()])))
        hb.fill_(SENTINEL)
        torch.cuda.synchronize()
        ctx.track_batch(P, 1, stb.data_ptr(), list(SLOT0), 3, 4, hb.data_ptr())
        env.sync()
        return hb.cpu().numpy()

    def pipelined_pair(between=None):
        stp.copy_(torch.from_numpy(env.start()))
        torch.cuda.synchronize()
        ctx.pipeline_begin(d[0])
        ctx.track_pipelined(P, 1, stp.data_ptr(), d[1])
        env.sync()
        a = stp.cpu().numpy().copy()
        if between:
            between()
        ctx.track_pipelined(P, 1, stp.data_ptr(), None)
        env.sync()
        return a, stp.cpu().numpy().copy()

    batch0 = prepared_batch()
    pipe0 = pipelined_pair()
    raw0 = env.alone(env.raw[0], 6, 1)
    env.check_lanes(env.raw, 6, 1, 4)
    before = env.captures()
    env.check_lanes([env.raw[2], env.raw[0], env.raw[1]], 6, 1, 4)
    assert env.captures() == before
    copies = [r.clone() for r in env.raw]
    hist, st = env.batch(copies, 6, 1, 4)
    assert env.captures() == before
    for b in range(3):
        ah, a_st = env.alone(env.raw[b], 6, 1)
        assert np.array_equal(hist[b], ah) and np.array_equal(st[b], a_st), b
    mid = []  # (track_raw_sequence would end the pipelined sequence: the batch alone runs here)
    pipe1 = pipelined_pair(between=lambda: mid.append(env.batch(env.raw, 6, 1, 4)))
    assert np.array_equal(pipe1[0], pipe0[0]) and np.array_equal(pipe1[1], pipe0[1])
    assert np.array_equal(mid[0][0], hist) and np.array_equal(mid[0][1], st)
    again = env.alone(env.raw[0], 6, 1, fresh=True)
    assert np.array_equal(again[0], raw0[0]) and np.array_equal(again[1], raw0[1])
    assert np.array_equal(prepared_batch(), batch0)


def test_all_zero_frame_in_one_lane(env):
    hist, _ = env.check_lanes([env.raw_hole, env.raw[1]], 3, 1, 4, equal_nan=True)
    assert np.isfinite(hist[1]).all()
    assert not np.array_equal(hist[0], env.alone(env.raw[0], 3, 1)[0], equal_nan=True)


def test_eval_count_is_the_lanes_sum(env):
    env.evals()
    total = 0
    for raw in env.raw:
        env.alone(raw, 3, 1, fresh=True)
        total += env.evals()
    assert total > 0
    env.batch(env.raw, 3, 1, 4)
    assert env.evals() == total


def test_preparation_results(env):
    """The lanes' prepared frames sit in buffers the call owns, and no entry point reads them
    back (hpe_frame_readback takes a slot), so the preparation is checked through the
    lane-alone equality only: after n = 2, each lane's last frame was prepared inside the batch's
    refine launch, and its {bestp, cost} equal those of the single sequence, whose preparation
    tests/test_gpu_prep.py compares with hpe.preprocess_depth bit for bit.  The host
    preprocessing of the same raw frames must differ between the lanes, so a lane that prepared
    another lane's frame could not pass."""
    hist, _ = env.check_lanes(env.raw, 2, 1, 4)
    pre = [env.hpe.preprocess_depth(env.depth[s][1], True, True) for s in range(3)]
    assert not np.array_equal(pre[0]["cloud"], pre[1]["cloud"])
    assert not np.array_equal(pre[1]["cloud"], pre[2]["cloud"])
    assert not np.array_equal(hist[0, 1], hist[1, 1]) and not np.array_equal(hist[1, 1], hist[2, 1])


def test_refusals_leave_the_context_usable(env):
    from hpe import _lib
    torch = env.torch
    st = torch.zeros((_lib.BATCH_MAX + 1, 27), dtype=torch.float64, device="cuda:0")
    call = env.lib.hpe_track_raw_batch_dev
    sp = C.c_void_p(st.data_ptr())
    r0 = env.raw[0].data_ptr()

    def err():
        return env.lib.hpe_last_error(env.ctx.h)

    def rc(B, ptrs, n=1, num_p=P, states=sp, downsample=1, focal=241.42, K=0):
        arr = (C.c_void_p * len(ptrs))(*ptrs) if ptrs is not None else None
        return call(env.ctx.h, num_p, 1, B, states, arr, n, 1, downsample, focal, K, None)

    env.check_lanes([env.raw[0]], 2, 1, 4)
    # every refusal returns its code and sets the message (the last call's text is kept)
    assert rc(0, [r0]) == _lib.HPE_E_ARG and b"lanes" in err()
    assert rc(_lib.BATCH_MAX + 1, [r0] * (_lib.BATCH_MAX + 1)) == _lib.HPE_E_ARG and b"lanes" in err()
    assert rc(1, [r0], states=None) == _lib.HPE_E_ARG and b"null" in err()
    assert rc(1, [r0], n=0) == _lib.HPE_E_ARG and b"n = 0" in err()
    assert rc(1, None) == _lib.HPE_E_ARG and b"null" in err()
    assert rc(2, [r0, None]) == _lib.HPE_E_ARG and b"lane 1" in err()
    assert rc(1, [r0], focal=0.0) == _lib.HPE_E_ARG and b"focal" in err()
    assert rc(1, [r0], focal=-1.0) == _lib.HPE_E_ARG and b"focal" in err()
    assert rc(1, [r0], K=-1) == _lib.HPE_E_ARG and b"frames_per_graph" in err()
    assert rc(1, [r0], K=33) == _lib.HPE_E_ARG and b"frames_per_graph" in err()
    assert rc(1, [r0], num_p=1024) == _lib.HPE_E_ARG and b"wave form" in err()
    assert rc(1, [r0], downsample=0) == _lib.HPE_E_ARG and b"downsample" in err()
    script = np.zeros((2, 2, 27))
    script[:, :, 26] = 1e300
    env.ctx.subswarm_init_scripted(script, 0)
    try:
        assert rc(1, [r0]) == _lib.HPE_E_STATE and b"transport" in err()   # a live transport
    finally:
        env.ctx.subswarm_fini()
    ext = torch.zeros(27, dtype=torch.float64, device="cuda:0")
    fn = _lib.EXCHANGE_FN(lambda user, d_ext, g: 0)
    env.ctx.check(env.lib.hpe_set_exchange(env.ctx.h, 2, C.c_void_p(ext.data_ptr()),
                                           C.cast(fn, C.c_void_p), None))
    try:
        assert rc(1, [r0]) == _lib.HPE_E_STATE and b"exchange" in err()    # hpe_set_exchange
    finally:
        env.ctx.check(env.lib.hpe_set_exchange(env.ctx.h, 0, None, None, None))
    env.check_lanes(env.raw, 6, 1, 4)
