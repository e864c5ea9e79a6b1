"""Wave-form lanes (hpe_set_batch_form(HPE_BATCH_FORM_WAVE)): the three batch calls with every
lane's pso_evolve in the wave-per-particle form.

Lane b of a wave-form batch must equal the batch call's single-sequence counterpart
(hpe_track_sequence_dev, hpe_track_raw_sequence_dev, hpe_pipeline_begin + hpe_track_pipelined) of
that lane alone on a context created under HPE_PSO_FORM=wave and HPE_PSO_WPP=<hpe_batch_wave_wpp
of the batch>, bit for bit: np.array_equal on whole histories and final states.  The yardstick
is always that single call, never the batch itself, and its waves per particle are the batch's:
the two forms are not assumed bit-identical to each other.

Both environment variables are read at hpe_create, so the file keeps a few contexts: the default
one (nothing set), the two yardsticks (wave, wpp 1 and 2) and two that only force HPE_PSO_WPP.
Frames are rendered once (hpe.synth.trajectory seeds 0, 1, 2, 250-point clouds) and prepared on
every context; a yardstick is computed once, shared and never changed.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NF = 5
SLOT0 = (10, 20, 30)       # the three sequences' first slots (250-point clouds)
FILT0 = (50, 60)           # two 2-frame sequences of 400-point clouds (stored)
EMPTY0 = 70                # sequence 0 with frame 1 empty
SENTINEL = -7.0


class Frames:
    """What every context is given: rendered once."""

    def __init__(self, ctx):
        import hpe
        import torch
        from hpe import synth
        self.depth = []
        for s in range(3):
            poses = synth.trajectory(NF, s)
            self.depth.append([np.ascontiguousarray(ctx.render_depth(th), dtype=np.float32)
                               for th in poses])
        self.filt = []  # the full cloud subsampled on the host to 400 points
        for s in range(2):
            for f in range(2):
                o = hpe.preprocess_depth(self.depth[s][f], True, False)
                assert len(o["cloud"]) > 400
                pick = np.linspace(0, len(o["cloud"]) - 1, 400).astype(int)
                self.filt.append((FILT0[s] + f, o, o["cloud"][pick]))
        self.raw = [torch.from_numpy(np.stack(d)).to("cuda:0") for d in self.depth]


class Env:
    """One context created under the given HPE_PSO_FORM / HPE_PSO_WPP (None: unset)."""

    def __init__(self, pool, form, wpp):
        import hpe
        import torch
        self.hpe, self.torch, self.pool = hpe, torch, pool
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
        self.pso = hpe.PSO()
        self.maxiter = None
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        if pool.frames is None:
            pool.frames = Frames(self.ctx)
        fr = pool.frames
        for s in range(3):
            for f, d in enumerate(fr.depth[s]):
                self.ctx.prepare_frame(SLOT0[s] + f, d)
        for slot, o, cloud in fr.filt:
            self.ctx.store_frame(slot, o["depth_cm"], o["dt"], cloud, o["scale"], o["dtmax"], o["K"])
        for f in range(3):
            d = fr.depth[0][f] if f != 1 else np.zeros_like(fr.depth[0][f])
            self.ctx.prepare_frame(EMPTY0 + f, d)
        self.sync()
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.h1 = torch.empty((NF, 27), dtype=torch.float64, device="cuda:0")
        self.bufs = {}  # (B, n) -> (states, hist): one buffer pair per shape (graph keys)

    def params(self, maxiter):
        if maxiter != self.maxiter:
            ub, lb, sd = self.hpe.reference_bounds()
            self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, maxiter, 1e-8, 1e-8)
            self.pso._push(self.ctx)
            self.maxiter = maxiter

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def start(self, x0=None):
        x = np.zeros(27)
        x[:26] = self.x0 if x0 is None else x0
        return x

    # ---- the single-sequence calls (the yardsticks, on a wave context; the block form on the
    # default one)
    def alone(self, kind, seq, n, refine, P, maxiter, x0=None):
        """(history n x 27, final state) of one sequence alone; live: (state after every frame,
        final state).  seq: a first slot (prepared), a sequence number (raw, live)."""
        self.params(maxiter)
        self.st1.copy_(self.torch.from_numpy(self.start(x0)))
        self.h1.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        if kind == "prepared":
            self.ctx.track_sequence(P, refine, self.st1.data_ptr(), seq, n, 2, self.h1.data_ptr())
        elif kind == "raw":
            self.ctx.track_raw_sequence(P, refine, self.st1.data_ptr(),
                                        self.pool.frames.raw[seq].data_ptr(), n,
                                        frames_per_graph=2, d_hist_ptr=self.h1.data_ptr())
        else:
            fr = self.pool.frames.depth[seq]
            out = []
            self.ctx.pipeline_begin(fr[0])
            for f in range(n):
                self.ctx.track_pipelined(P, refine, self.st1.data_ptr(), fr[f + 1] if f + 1 < n else None)
                self.sync()
                out.append(self.st1.cpu().numpy().copy())
            return np.array(out), out[-1]
        self.sync()
        return self.h1.cpu().numpy()[:n].copy(), self.st1.cpu().numpy().copy()

    # ---- the batch calls
    def batch(self, kind, seqs, n, refine, K, P, maxiter, form="wave", x0s=None):
        """(history B x n x 27, states B x 27) of the batch over the lanes' sequences."""
        self.params(maxiter)
        B = len(seqs)
        if (B, n) not in self.bufs:
            self.bufs[(B, n)] = (self.torch.zeros((B, 27), dtype=self.torch.float64, device="cuda:0"),
                                 self.torch.empty((B, n, 27), dtype=self.torch.float64, device="cuda:0"))
        st, hist = self.bufs[(B, n)]
        x = np.stack([self.start(None if x0s is None else x0s[b]) for b in range(B)])
        st.copy_(self.torch.from_numpy(x))
        hist.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        self.ctx.set_batch_form(form)
        try:
            if kind == "prepared":
                self.ctx.track_batch(P, refine, st.data_ptr(), seqs, n, K, hist.data_ptr())
            else:
                raws = [self.pool.frames.raw[s].data_ptr() for s in seqs]
                self.ctx.track_raw_batch(P, refine, st.data_ptr(), raws, n, frames_per_graph=K,
                                         d_hist_ptr=hist.data_ptr())
            self.sync()
        finally:
            self.ctx.set_batch_form("auto")
        return hist.cpu().numpy(), st.cpu().numpy()


class Pool:
    def __init__(self):
        self.frames = None
        self.envs = {}
        self.yard = {}

    def env(self, form=None, wpp=None):
        if (form, wpp) not in self.envs:
            self.envs[(form, wpp)] = Env(self, form, wpp)
        return self.envs[(form, wpp)]

    def yardstick(self, wpp, kind, seq, n, refine, P, maxiter, x0=None):
        key = (wpp, kind, seq, n, refine, P, maxiter, None if x0 is None else tuple(x0))
        if key not in self.yard:
            self.yard[key] = self.env("wave", wpp).alone(kind, seq, n, refine, P, maxiter, x0)
        return self.yard[key]

    def check_lanes(self, env, kind, seqs, n, refine, K, P, maxiter, x0s=None, equal_nan=False):
        """A wave-form batch on env against every lane's yardstick of the batch's wpp."""
        wpp = env.ctx.batch_wave_wpp(P, len(seqs))
        assert wpp in (1, 2)
        hist, st = env.batch(kind, seqs, n, refine, K, P, maxiter, "wave", x0s)
        for b, s in enumerate(seqs):
            ah, a_st = self.yardstick(wpp, kind, s, n, refine, P, maxiter,
                                      None if x0s is None else x0s[b])
            assert np.array_equal(hist[b], ah, equal_nan=equal_nan), (b, s, wpp)
            assert np.array_equal(st[b], a_st, equal_nan=equal_nan), (b, s, wpp)
        return hist, st

    def close(self):
        for e in self.envs.values():
            e.ctx.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


@pytest.mark.parametrize("refine", [1, 0])
@pytest.mark.parametrize("wpp", [1, 2])
def test_tail_waves_chunk_and_tail(pool, wpp, refine):
    """B = 3 distinct lanes, P = 30 (no multiple of 4, nor of 2: the last workgroup of a lane has
    invalid waves at wpp 1 and an invalid pair at wpp 2), maxiter 7, 5 frames in chunks of 2: two
    full chunks and a 1-frame tail.  The batch context only forces HPE_PSO_WPP.  The same call
    again replays: it captures nothing and gives the same bits."""
    env = pool.env(None, wpp)
    assert env.ctx.batch_wave_wpp(30, 3) == wpp
    hist, st = pool.check_lanes(env, "prepared", list(SLOT0), 5, refine, 2, 30, 7)
    assert not (hist == SENTINEL).any()
    assert not np.array_equal(hist[0], hist[1]) and not np.array_equal(hist[1], hist[2])
    before = env.ctx.graph_captures()
    hist2, st2 = pool.check_lanes(env, "prepared", list(SLOT0), 5, refine, 2, 30, 7)
    assert env.ctx.graph_captures() == before
    assert np.array_equal(hist2, hist) and np.array_equal(st2, st)


def test_lane_order(pool):
    env = pool.env()
    a, _ = pool.check_lanes(env, "prepared", list(SLOT0), 5, 1, 2, 64, 7)
    b, _ = pool.check_lanes(env, "prepared", [SLOT0[2], SLOT0[0], SLOT0[1]], 5, 1, 2, 64, 7)
    assert np.array_equal(b[0], a[2]) and np.array_equal(b[1], a[0]) and np.array_equal(b[2], a[1])


def test_one_sequence_from_three_poses(pool):
    env = pool.env()
    x1, x2 = env.x0.copy(), env.x0.copy()
    x1[3:6] += (0.4, -0.3, 0.5)
    x1[6:] += 1.5
    x2[0:3] += (2.0, -1.0, 1.5)
    hist, _ = pool.check_lanes(env, "prepared", [SLOT0[0]] * 3, 5, 1, 2, 64, 7, x0s=[env.x0, x1, x2])
    assert not np.array_equal(hist[0], hist[1]) and not np.array_equal(hist[1], hist[2])
    assert not np.array_equal(hist[0], hist[2])


def test_the_wpp_rule(pool):
    """HPE_PSO_WPP unset: two waves per particle while B * num_p <= 1024, one beyond -- each
    checked against the yardstick of that wpp."""
    env = pool.env()
    assert env.ctx.batch_wave_wpp(64, 3) == 2
    assert env.ctx.batch_wave_wpp(256, 5) == 1
    assert env.ctx.batch_wave_wpp(256, 4) == 2 and env.ctx.batch_wave_wpp(1024, 1) == 2
    assert env.ctx.batch_wave_wpp(1025, 1) == 1
    pool.check_lanes(env, "prepared", list(SLOT0), 5, 1, 2, 64, 7)
    slots = [SLOT0[b % 3] for b in range(5)]
    pool.check_lanes(env, "prepared", slots, 2, 1, 2, 256, 4)
    # a forced value wins over the rule
    assert pool.env(None, 1).ctx.batch_wave_wpp(64, 3) == 1
    assert pool.env(None, 2).ctx.batch_wave_wpp(256, 5) == 2


def test_large_swarms(pool):
    """num_p = 1024: refused under AUTO as before, tracked under WAVE."""
    from hpe import _lib
    env = pool.env()
    env.params(4)
    st = env.torch.zeros((2, 27), dtype=env.torch.float64, device="cuda:0")
    arr = (C.c_int32 * 2)(SLOT0[0], SLOT0[1])
    rc = env.lib.hpe_track_batch_dev(env.ctx.h, 1024, 1, 2, C.c_void_p(st.data_ptr()), arr, 2, 0, None)
    assert rc == _lib.HPE_E_ARG
    assert b"wave form" in env.lib.hpe_last_error(env.ctx.h)
    assert env.ctx.batch_wave_wpp(1024, 2) == 1
    pool.check_lanes(env, "prepared", [SLOT0[0], SLOT0[1]], 2, 1, 2, 1024, 4)


def test_filter_clouds(pool):
    """400-point clouds: the final kernel's FILT form."""
    hist, _ = pool.check_lanes(pool.env(), "prepared", list(FILT0), 2, 1, 2, 64, 7)
    assert not np.array_equal(hist[0], hist[1])


def test_empty_frame_in_one_lane(pool):
    hist, _ = pool.check_lanes(pool.env(), "prepared", [EMPTY0, SLOT0[1]], 3, 1, 2, 64, 7,
                               equal_nan=True)
    assert np.isnan(hist[0, 1, 26]) and not np.isnan(hist[1]).any()


def test_raw_batch(pool):
    """hpe_track_raw_batch_dev: B = 3, 5 frames in chunks of 2."""
    hist, _ = pool.check_lanes(pool.env(), "raw", [0, 1, 2], 5, 1, 2, 64, 7)
    assert not (hist == SENTINEL).any()


def test_live_batch_and_a_form_change_inside_it(pool):
    """The live pair: B = 3, 4 frames, the states compared after every frame.  A live batch keeps
    the form it began with: another form is HPE_E_STATE while it is in progress (nothing changes),
    its own form is accepted, and after the batch ended the form is free again."""
    from hpe import _lib
    env = pool.env()
    P, n, names = 64, 4, [0, 1, 2]
    env.params(7)
    wpp = env.ctx.batch_wave_wpp(P, 3)
    fr = pool.frames.depth
    st = env.torch.zeros((3, 27), dtype=env.torch.float64, device="cuda:0")
    st.copy_(env.torch.from_numpy(np.stack([env.start()] * 3)))
    env.torch.cuda.synchronize()
    env.ctx.set_batch_form("wave")
    try:
        env.ctx.batch_pipeline_begin([fr[s][0] for s in names])
        got = []
        for f in range(n):
            env.ctx.track_batch_pipelined(P, 1, st.data_ptr(),
                                          [fr[s][f + 1] for s in names] if f + 1 < n else None)
            env.sync()
            got.append(st.cpu().numpy().copy())
            if f == 1:
                assert env.lib.hpe_set_batch_form(env.ctx.h, _lib.BATCH_FORM_AUTO) == _lib.HPE_E_STATE
                assert b"live batch" in env.lib.hpe_last_error(env.ctx.h)
                assert env.lib.hpe_set_batch_form(env.ctx.h, _lib.BATCH_FORM_WAVE) == _lib.HPE_OK
    finally:
        # the batch ended with its last frame (or never began): the form is free
        rc_after = env.lib.hpe_set_batch_form(env.ctx.h, _lib.BATCH_FORM_AUTO)
    assert rc_after == _lib.HPE_OK
    for b, s in enumerate(names):
        want, _ = pool.yardstick(wpp, "live", s, n, 1, P, 7)
        for f in range(n):
            assert np.array_equal(got[f][b], want[f]), (b, f)


def test_no_stale_graph_between_the_forms(pool):
    """One default context, the same buffers and shape: AUTO (the block-form single path of that
    context), WAVE (the wave yardstick), AUTO again -- which replays the first run's graphs."""
    env = pool.env()
    seqs, n, K, P, G = list(SLOT0), 5, 2, 64, 7
    block = [env.alone("prepared", s, n, 1, P, G) for s in seqs]

    def check_block():
        hist, st = env.batch("prepared", seqs, n, 1, K, P, G, form="auto")
        for b in range(3):
            assert np.array_equal(hist[b], block[b][0]) and np.array_equal(st[b], block[b][1])
        return hist

    check_block()
    pool.check_lanes(env, "prepared", seqs, n, 1, K, P, G)
    before = env.ctx.graph_captures()
    check_block()
    assert env.ctx.graph_captures() == before
    pool.check_lanes(env, "prepared", seqs, n, 1, K, P, G)
    assert env.ctx.graph_captures() == before


def test_argument_errors(pool):
    from hpe import _lib
    env = pool.env()
    lib = env.lib
    for bad in (2, -1):
        assert lib.hpe_set_batch_form(env.ctx.h, bad) == _lib.HPE_E_ARG
        assert b"batch form" in lib.hpe_last_error(env.ctx.h)
    assert lib.hpe_set_batch_form(None, _lib.BATCH_FORM_WAVE) == _lib.HPE_E_ARG
    assert lib.hpe_batch_wave_wpp(None, 64, 3) == _lib.HPE_E_ARG
    assert lib.hpe_batch_wave_wpp(env.ctx.h, 0, 3) == _lib.HPE_E_ARG
    assert lib.hpe_batch_wave_wpp(env.ctx.h, 64, 0) == _lib.HPE_E_ARG
    assert lib.hpe_batch_wave_wpp(env.ctx.h, 64, _lib.BATCH_MAX + 1) == _lib.HPE_E_ARG
    with pytest.raises(ValueError):
        env.ctx.set_batch_form("block")
    # the refused values changed nothing: the default form still refuses the wave form
    env.params(4)
    st = env.torch.zeros((1, 27), dtype=env.torch.float64, device="cuda:0")
    arr = (C.c_int32 * 1)(SLOT0[0])
    assert lib.hpe_track_batch_dev(env.ctx.h, 1024, 1, 1, C.c_void_p(st.data_ptr()), arr, 1, 0,
                                   None) == _lib.HPE_E_ARG
