"""Batched tracking (hpe_track_batch_dev): B independent sequences in the same launches.

Lane b of a batch must equal hpe_track_sequence_dev of that lane alone on the same context,
bit for bit: np.array_equal on the whole n x 27 history and on the final state.  The
single-sequence path is the yardstick, never the batch itself.  Small shapes: P = 64,
maxiter 7 (G = 6), at most 7 synthetic frames per sequence (hpe.synth.trajectory seeds 0, 1,
2, rendered and device-prepared), one context for the whole file.

The ROW16 = false kernels (informant in-degree above 15) have no case here: under seed 1000
no swarm size of the workgroup form (P < 1024) reaches an in-degree above 14 for G = 3, 6 or
30 (hpe::make_links searched on the host).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER, NF = 64, 7, 7
SLOT0 = (10, 20, 30)       # the three sequences' first slots (250-point clouds)
FILT0 = (50, 60)           # two 2-frame sequences of 400-point clouds (stored)
EMPTY0 = 70                # sequence 0 with frame 1 empty
FULL0 = 80                 # one full-cloud frame (not down-sampled)
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
            for f, d in enumerate(self.depth[s]):
                self.ctx.prepare_frame(SLOT0[s] + f, d)
        for s in range(2):  # FILT: the full cloud subsampled on the host to 400 points
            for f in range(2):
                o = hpe.preprocess_depth(self.depth[s][f], True, False)
                cloud = o["cloud"]
                assert len(cloud) > 400
                pick = np.linspace(0, len(cloud) - 1, 400).astype(int)
                self.ctx.store_frame(FILT0[s] + f, o["depth_cm"], o["dt"], cloud[pick],
                                     o["scale"], o["dtmax"], o["K"])
        for f in range(3):
            d = self.depth[0][f] if f != 1 else np.zeros_like(self.depth[0][f])
            self.ctx.prepare_frame(EMPTY0 + f, d)
        self.ctx.prepare_frame(FULL0, self.depth[0][0], downsample=False)
        self.sync()
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.h1 = torch.empty((NF, 27), dtype=torch.float64, device="cuda:0")
        self.bufs = {}    # (B, n) -> (states, hist): one buffer pair per shape (graph keys)
        self._alone = {}  # computed once, shared, never changed

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

    def alone(self, slot0, n, refine, x0=None, fresh=False):
        """track_sequence of one lane alone: (history n x 27, final state)."""
        exact = self.ctx.refine_exact
        key = (slot0, n, refine, exact, None if x0 is None else tuple(x0))
        if fresh or key not in self._alone:
            self.st1.copy_(self.torch.from_numpy(self.start(x0)))
            self.h1.fill_(SENTINEL)
            self.torch.cuda.synchronize()
            self.ctx.track_sequence(P, refine, self.st1.data_ptr(), slot0, n, 4, self.h1.data_ptr())
            self.sync()
            r = (self.h1.cpu().numpy()[:n].copy(), self.st1.cpu().numpy().copy())
            if fresh:
                return r
            self._alone[key] = r
        return self._alone[key]

    def batch(self, slots, n, refine, K, x0s=None, num_p=P):
        """track_batch over the lanes' first slots: (history B x n x 27, states B x 27)."""
        B = len(slots)
        if (B, n) not in self.bufs:
            self.bufs[(B, n)] = (self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0"),
                                 self.torch.empty((B, n, 27), dtype=self.torch.float64, device="cuda:0"))
        st, hist = self.bufs[(B, n)]
        x = np.stack([self.start(None if x0s is None else x0s[b]) for b in range(B)])
        st.copy_(self.torch.from_numpy(x))
        hist.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        self.ctx.track_batch(num_p, refine, st.data_ptr(), slots, n, K, hist.data_ptr())
        self.sync()
        return hist.cpu().numpy(), st.cpu().numpy()

    def check_lanes(self, slots, n, refine, K, x0s=None, equal_nan=False):
        hist, st = self.batch(slots, n, refine, K, x0s)
        for b, s0 in enumerate(slots):
            ah, a_st = self.alone(s0, n, refine, None if x0s is None else x0s[b])
            assert np.array_equal(hist[b], ah, equal_nan=equal_nan), (b, s0)
            assert np.array_equal(st[b], a_st, equal_nan=equal_nan), (b, s0)
        return hist, st


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


@pytest.mark.parametrize("refine", [1, 0])
def test_three_lanes_chunk_and_tail(env, refine):
    """B = 3 distinct sequences, n = 6 in chunks of 4: a full chunk and a 2-frame tail chunk,
    the cursors crossing a graph boundary."""
    hist, _ = env.check_lanes(list(SLOT0), 6, refine, 4)
    assert not np.array_equal(hist[0], hist[1]) and not np.array_equal(hist[1], hist[2])
    assert not (hist == SENTINEL).any()


@pytest.mark.parametrize("exact", [False, True])
def test_both_refine_forms(env, exact):
    was = env.ctx.refine_exact
    env.ctx.refine_exact = exact
    try:
        env.check_lanes(list(SLOT0), 6, 1, 4)
    finally:
        env.ctx.refine_exact = was


def test_one_lane_is_track_sequence(env):
    env.check_lanes([SLOT0[1]], 6, 1, 4)


def test_two_lanes_on_the_same_slots(env):
    """Two hands in one depth stream: the same slot range, different x0."""
    x1 = env.x0.copy()
    x1[3:6] += (0.4, -0.3, 0.5)
    x1[6:] += 1.5
    hist, _ = env.check_lanes([SLOT0[0], SLOT0[0]], 5, 1, 4, x0s=[env.x0, x1])
    assert not np.array_equal(hist[0], hist[1])


def test_full_batch(env):
    from hpe import _lib
    slots = [SLOT0[b % 3] for b in range(_lib.BATCH_MAX)]
    env.check_lanes(slots, 2, 1, 1)


def test_graph_reuse_over_permuted_slots(env):
    """Chunk graphs are keyed by shape: the same call over permuted slot ranges captures
    nothing, and the single-sequence path still works and still gives its earlier bits."""
    env.check_lanes(list(SLOT0), 6, 1, 4)
    before = env.captures()
    env.check_lanes([SLOT0[2], SLOT0[0], SLOT0[1]], 6, 1, 4)
    assert env.captures() == before
    again = env.alone(SLOT0[0], 6, 1, fresh=True)
    first = env.alone(SLOT0[0], 6, 1)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


def test_filt_form(env):
    """400-point clouds: above HPE_NT / 2 (the FILT kernels), below the staged refine's bound."""
    hist, _ = env.check_lanes(list(FILT0), 2, 1, 8)
    assert not np.array_equal(hist[0], hist[1])


def test_empty_frame_in_one_lane(env):
    hist, _ = env.check_lanes([EMPTY0, SLOT0[1]], 3, 1, 4, equal_nan=True)
    assert np.isnan(hist[0, 1, 26]) and not np.isnan(hist[1]).any()


def test_eval_count_is_the_lanes_sum(env):
    env.evals()
    total = 0
    for s0 in SLOT0:
        env.alone(s0, 3, 1, fresh=True)
        total += env.evals()
    assert total > 0
    env.batch(list(SLOT0), 3, 1, 4)
    assert env.evals() == total


def test_refusals_leave_the_context_usable(env):
    from hpe import _lib
    st = env.torch.zeros((_lib.BATCH_MAX + 1, 27), dtype=env.torch.float64, device="cuda:0")
    call = env.lib.hpe_track_batch_dev
    sp = C.c_void_p(st.data_ptr())

    def rc(B, slots, n=1, num_p=P):
        arr = (C.c_int32 * max(len(slots), 1))(*slots)
        return call(env.ctx.h, num_p, 1, B, sp, arr, n, 0, None)

    assert rc(0, [SLOT0[0]]) == _lib.HPE_E_ARG
    assert rc(_lib.BATCH_MAX + 1, [SLOT0[0]] * (_lib.BATCH_MAX + 1)) == _lib.HPE_E_ARG
    assert rc(1, [FULL0]) == _lib.HPE_E_ARG                       # n_max > RF_STAGE_MAX
    assert rc(2, [SLOT0[0], FILT0[0]], n=2) == _lib.HPE_E_ARG     # lanes disagree on FILT
    assert rc(1, [SLOT0[0]], num_p=1024) == _lib.HPE_E_ARG        # the wave form
    assert rc(1, [4000]) == _lib.HPE_E_ARG                        # no frame there
    assert env.lib.hpe_last_error(env.ctx.h)
    script = np.zeros((2, 2, 27))
    script[:, :, 26] = 1e300
    env.ctx.subswarm_init_scripted(script, 0)
    try:
        assert rc(1, [SLOT0[0]]) == _lib.HPE_E_STATE              # a live transport
    finally:
        env.ctx.subswarm_fini()
    env.check_lanes(list(SLOT0), 6, 1, 4)
