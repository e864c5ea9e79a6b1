"""A tracking call leaves nothing behind that changes what the next call of another form computes.

Seen from outside only: the tracking forms run one after the other on one context, and every
state and history row must equal, bit for bit, the same call made alone on a fresh context.
What a call enqueues (descriptor, cursor, history, frame counter, the exchange's deferred pick)
must reach its launches with the call and end with it.

Smallest shapes that still run every launch of a frame: P = 32, maxiter 3 (G = 2), three
250-point synthetic frames of synth.trajectory(3, 0), frames_per_graph = 2 (one chunk of two
frames and one tail), every call from hpe.X0.  Slot 3 holds frame 0 again, so that the second
lane of the batch tracks frames 1, 2, 0.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_subswarm_world import _same, _table_script

pytestmark = pytest.mark.gpu

P, MAXITER, N, K = 32, 3, 3, 2
SENTINEL = -7.0  # history rows no frame has written


@pytest.fixture(scope="module")
def frames():
    """(poses, depth frames) of the trajectory, rendered once."""
    import hpe
    from hpe import synth
    poses = synth.trajectory(N, 0)
    hand = hpe.reference_hand(device=0)
    depth = [np.ascontiguousarray(hand.ctx.render_depth(th)) for th in poses]
    hand.ctx.close()
    return poses, depth


class Rig:
    """One fresh context with the frames device-prepared in slots 0..3 (slot 3: frame 0 again),
    seeded `seed`; one state buffer of two lanes and one history buffer for every call (graph
    keys)."""

    def __init__(self, depth, seed=1000):
        import hpe
        import torch
        self.hpe, self.torch = hpe, torch
        self.hand = hpe.reference_hand(device=0)
        self.ctx = self.hand.ctx
        ub, lb, sd = hpe.reference_bounds()
        pso = hpe.PSO()
        pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        pso.seed = seed
        pso._push(self.ctx)
        self.depth = depth
        for f in range(N + 1):
            self.ctx.prepare_frame(f, depth[f % N])
        self.raw = torch.from_numpy(np.stack(depth).astype(np.float32)).to("cuda:0")
        self.x0 = np.zeros(27)
        self.x0[:26] = np.asarray(hpe.X0, dtype=np.float64)
        self.st = torch.zeros((2, 27), dtype=torch.float64, device="cuda:0")
        self.hist = torch.empty((2 * N, 27), dtype=torch.float64, device="cuda:0")
        self.sync()

    def sync(self):
        self.ctx.check(self.ctx.lib.hpe_sync(self.ctx.h))

    def close(self):
        self.ctx.close()

    def reset(self, x0=None):
        self.sync()
        x = self.torch.from_numpy(self.x0 if x0 is None else x0)
        self.st.copy_(x.expand_as(self.st))
        self.hist.fill_(SENTINEL)
        self.torch.cuda.synchronize()

    def _out(self, lanes=1, hist=True):
        """The rows a call wrote: its history rows (if it has any), then its final states."""
        self.sync()
        rows = [self.st[:lanes].cpu().numpy().copy()]
        if hist:
            rows.insert(0, self.hist[:lanes * N].cpu().numpy().copy())
        r = np.concatenate(rows)
        assert np.isfinite(r).all() and not (r == SENTINEL).any()
        return r

    # ---- the calls: each from x0, each returns every row it wrote
    def frame(self, slot=0, x0=None):
        self.reset(x0)
        self.ctx.select_frame(slot)
        self.ctx.check(self.ctx.lib.hpe_track_frame_dev(self.ctx.h, P, 1,
                                                        C.c_void_p(self.st.data_ptr())))
        return self._out(hist=False)

    def sequence(self):
        self.reset()
        self.ctx.track_sequence(P, 1, self.st.data_ptr(), 0, N, K, self.hist.data_ptr())
        return self._out()

    def pipelined(self):
        self.reset()
        self.ctx.pipeline_begin(self.depth[0])
        rows = []
        for f in range(N):
            self.ctx.track_pipelined(P, 1, self.st.data_ptr(),
                                     self.depth[f + 1] if f + 1 < N else None)
            rows.append(self._out(hist=False))
        return np.concatenate(rows)

    def raw_sequence(self):
        self.reset()
        self.ctx.track_raw_sequence(P, 1, self.st.data_ptr(), self.raw.data_ptr(), N,
                                    frames_per_graph=K, d_hist_ptr=self.hist.data_ptr())
        return self._out()

    def batch(self):
        self.reset()
        self.ctx.track_batch(P, 1, self.st.data_ptr(), [0, 1], N, K, self.hist.data_ptr())
        return self._out(lanes=2)

    def evolve(self, slot=None):
        """hpe_pso_evolve on the selected frame (slot: select it first)."""
        if slot is not None:
            self.ctx.select_frame(slot)
        dp = self.hpe._lib.dp
        x, out, bc = self.x0[:26].copy(), np.zeros(27), C.c_double(0)
        self.ctx.check(self.ctx.lib.hpe_pso_evolve(self.ctx.h, x.ctypes.data_as(dp), P,
                                                   out.ctypes.data_as(dp), C.byref(bc)))
        out[26] = bc.value
        assert np.isfinite(out).all()
        return out

    def refine(self, slot=None):
        """hpe_refine_init_pose on the selected frame (slot: select it first)."""
        if slot is not None:
            self.ctx.select_frame(slot)
        x, ev = self.x0[:26].copy(), C.c_int32(0)
        self.ctx.check(self.ctx.lib.hpe_refine_init_pose(
            self.ctx.h, x.ctypes.data_as(self.hpe._lib.dp), C.byref(ev)))
        assert np.isfinite(x).all() and not np.array_equal(x, self.x0[:26])
        return np.append(x, ev.value)


def _alone(depth, call, *args, **kw):
    """The call on a context that has run nothing else."""
    r = Rig(depth, **kw)
    try:
        return getattr(r, call)(*args)
    finally:
        r.close()


def test_every_form_after_every_other_without_exchange(frames):
    """hpe_track_frame_dev, hpe_track_sequence_dev (then hpe_pso_evolve and hpe_refine_init_pose
    on the frame the sequence left selected: its last), the pipelined loop,
    hpe_track_raw_sequence_dev, hpe_track_batch_dev with two lanes and hpe_track_frame_dev again,
    on one context: each gives the bits it gives alone."""
    _, depth = frames
    T = Rig(depth)
    got = [("frame", T.frame()), ("sequence", T.sequence()), ("evolve", T.evolve()),
           ("refine", T.refine()), ("pipelined", T.pipelined()),
           ("raw_sequence", T.raw_sequence()), ("batch", T.batch()), ("frame", T.frame())]
    T.close()
    alone = {"evolve": _alone(depth, "evolve", N - 1), "refine": _alone(depth, "refine", N - 1)}
    for call, rows in got:
        if call not in alone:
            alone[call] = _alone(depth, call)
        assert rows.shape == alone[call].shape and np.array_equal(rows, alone[call]), call
    # the forms agree where they track the same frames (the rows are not trivially equal)
    assert np.array_equal(alone["sequence"][:N], alone["pipelined"])
    assert np.array_equal(alone["batch"][:N], alone["sequence"][:N])
    assert not np.array_equal(alone["batch"][N], alone["batch"][0])


WORLD, RANK = 2, 1


@pytest.fixture(scope="module")
def script(frames):
    """(script, x): the peer (rank 0) wins frame 0, loses frame 1 and ties frame 2 (the lower
    rank wins), built from this rank's own rows on a context without a transport; x: the picked
    rows.  As tests/test_gpu_subswarm_world.py builds it."""
    import torch
    from hpe.dist import pick_best, subswarm_seed
    poses, depth = frames
    make = _table_script([{0: ("x", 0.5)}, {}, {0: "tie"}], WORLD, RANK)
    E = Rig(depth, seed=subswarm_seed(RANK))
    sc, xs, x = [], [], None
    for f in range(N):
        own = E.frame(f, x)[0]
        rows = np.array(make(f, own, poses[f]), dtype=np.float64)
        sc.append(rows.copy())
        rows[RANK] = own
        x = pick_best(torch.from_numpy(rows)).numpy().copy()
        xs.append(x)
    E.close()
    sc, xs = np.array(sc), np.array(xs)
    assert _same(xs[0], sc[0, 0]) and _same(xs[2], sc[2, 0]) and not _same(xs[1], sc[1, 0])
    return sc, xs


@pytest.mark.parametrize("direct", [False, True], ids=["captured", "direct"])
def test_forms_in_either_order_with_the_scripted_exchange(frames, script, direct):
    """World 2, rank 1, the script rewound before every call (a script of the same shape
    reloaded): hpe_track_sequence_dev (frame 0's pick inside frame 1's refine launch, frames 1
    and 2 by k_pick_best), the pipelined loop and hpe_track_frame_dev give the same bits in this
    order on one context and in the reverse order on another -- captured, and launched directly
    (hpe_subswarm_enable(ctx, 2)).  A pick carried from one call into the next would show here."""
    from hpe.dist import subswarm_seed
    _, depth = frames
    sc, x = script
    order = ("sequence", "pipelined", "frame")
    got = []
    for calls in (order, order[::-1]):
        T = Rig(depth, seed=subswarm_seed(RANK))
        T.ctx.subswarm_init_scripted(sc, RANK)
        if direct:
            T.ctx.subswarm_enable(True, direct=True)
        assert T.ctx.subswarm_info()["in_graphs"] == (not direct)
        res = {}
        for call in calls:
            T.ctx.subswarm_init_scripted(sc, RANK)  # rewound
            res[call] = getattr(T, call)()
        assert (T.ctx.graph_captures() == 0) == direct
        T.close()
        got.append(res)
    for call in order:
        assert _same(got[0][call], got[1][call]), call
    # the exchange acted: the sequence's history is the picked rows, the other forms agree
    assert _same(got[0]["sequence"][:N], x)
    assert _same(got[0]["pipelined"], x) and _same(got[0]["frame"][0], x[0])
