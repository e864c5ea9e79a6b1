"""The subswarm exchange with more than one rank, on one GPU (hpe_subswarm_init_scripted).

RCCL refuses two ranks on one device, so the library's per-frame exchange had only run at
world 1, where the pick always takes row 0 and that row is the rank's own: a wrong row
offset, a wrong tie rule or a refine that starts from the stale d_state gives the correct
code's bits.  The scripted transport puts peers' rows where the all-gather would have, and
everything downstream of "the gather buffer holds N rows" is the RCCL transport's own code:
k_pso_final writing gather row `rank`, the pick inside the next frame's k_refine (every frame
of a chunk but the last), the chunk-end k_pick_best with the history row.

Expected values use no exchange code: a second context WITHOUT a transport (same seed
1000 + rank) tracks each frame with hpe_track_frame_dev from x_{f-1} -- this rank's own row,
a path checked against the oracle and bit-identical to every chunked form
(test_gpu_prep.py) -- the script frame is built from that row (ties carry its cost bits), and
x_f = hpe.dist.pick_best(rows) (NaN -> +inf, first argmin).  The run under test replays the
finished script; every history row and the final state must equal x_f BIT FOR BIT, NaNs
included (own rows come from kernels bit-identical across forms; peer rows are copied).

The script's row `rank` (never to be copied) holds a poison: an in-bounds pose with cost
-1e300, which would win every pick but a -inf one if the copy kernel wrote it.
"""
import ctypes as C

import numpy as np
import pytest

import hand_data
from hand_data import REFINE_RIGID
import oracle_np

pytestmark = pytest.mark.gpu

POSE_TOL, COST_RTOL = 1e-6, 1e-8  # tests/test_gpu_configs.py
SENTINEL = -7.0  # history rows no frame has written


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _peer_pose(truth, w):
    """Rank w's scripted pose: the trajectory's true pose plus a fixed offset (4 deg, 1.5 cm,
    3 deg per joint, scaled by rank), clipped into reference_bounds()."""
    ub, lb, _ = oracle_np.reference_bounds()
    off = np.zeros(26)
    off[0:3], off[3:6], off[6:] = 4.0, 1.5, 3.0
    return np.clip(truth + (1.0 + 0.125 * w) * off, lb, ub)


def _table_script(table, world, rank, default=("x", 2.0)):
    """make(f, own, truth) -> (world, 27) script frame.  table[f] maps a peer rank to its
    cost: "tie" (the own cost's bits), ("x", m) (m times the own cost) or ("v", value);
    the other peers get `default`."""
    def make(f, own, truth):
        rows = np.empty((world, 27))
        for w in range(world):
            rows[w, :26] = _peer_pose(truth, w)
            spec = table[f].get(w, default)
            rows[w, 26] = own[26] if spec == "tie" else (spec[1] * own[26] if spec[0] == "x"
                                                         else spec[1])
        rows[rank, :26] = oracle_np.X0  # the poison row: never copied
        rows[rank, 26] = -1e300
        return rows
    return make


def _frames(np_hand, n, seed, empty=()):
    poses = hand_data.trajectory(n, seed=seed)
    depth = [oracle_np.render_depth_mm(np_hand, th) for th in poses]
    for f in empty:
        depth[f] = np.zeros_like(depth[f])
    return poses, depth


class Rig:
    """One fresh context (the kernel-form switches are read at hpe_create) with the frames
    device-prepared in slots 0..n-1, seeded 1000 + rank; one state and one history buffer
    (graph keys)."""

    def __init__(self, depth, P, maxiter, rank, refine=1, downsample=True, exact=None):
        import hpe
        import torch
        from hpe.dist import subswarm_seed
        self.torch = torch
        self.hand = hpe.reference_hand(device=0)
        self.ctx = self.hand.ctx
        if exact is not None:
            self.ctx.refine_exact = exact
        ub, lb, sd = oracle_np.reference_bounds()
        pso = hpe.PSO()
        pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, maxiter, 1e-8, 1e-8)
        pso.seed = subswarm_seed(rank)
        pso._push(self.ctx)
        self.P, self.rank, self.refine, self.ds = P, rank, refine, downsample
        self.depth, self.n = depth, len(depth)
        for f, d in enumerate(depth):
            self.ctx.prepare_frame(f, d, downsample=downsample)
        self.sync()
        self.st = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.hist = torch.empty((self.n, 27), dtype=torch.float64, device="cuda:0")
        self.d_raw = None

    def sync(self):
        self.ctx.check(self.ctx.lib.hpe_sync(self.ctx.h))

    def close(self):
        self.ctx.close()

    def reset(self, x0=None):
        x = np.zeros(27)
        x[:26] = oracle_np.X0
        self.st.copy_(self.torch.from_numpy(x if x0 is None else x0))
        self.hist.fill_(SENTINEL)
        self.torch.cuda.synchronize()

    def _frame(self, f):
        self.ctx.select_frame(f)
        self.ctx.check(self.ctx.lib.hpe_track_frame_dev(self.ctx.h, self.P, self.refine,
                                                        C.c_void_p(self.st.data_ptr())))
        self.sync()
        return self.st.cpu().numpy().copy()

    # ---- the tracking forms: each returns (history rows, final state)
    def frame_dev(self, n=None):
        self.reset()
        rows = np.array([self._frame(f) for f in range(n or self.n)])
        return rows, rows[-1]

    def seq(self, K, n=None, hist=True):
        self.reset()
        self.ctx.track_sequence(self.P, self.refine, self.st.data_ptr(), 0, n or self.n, K,
                                self.hist.data_ptr() if hist else None)
        self.sync()
        return self.hist.cpu().numpy()[:n or self.n], self.st.cpu().numpy()

    def raw(self, K):
        if self.d_raw is None:
            self.d_raw = self.torch.from_numpy(np.stack(self.depth).astype(np.float32)).to("cuda:0")
        self.reset()
        self.ctx.track_raw_sequence(self.P, self.refine, self.st.data_ptr(),
                                    self.d_raw.data_ptr(), self.n, downsample=self.ds,
                                    frames_per_graph=K, d_hist_ptr=self.hist.data_ptr())
        self.sync()
        return self.hist.cpu().numpy(), self.st.cpu().numpy()

    def pipelined(self):
        self.reset()
        self.ctx.pipeline_begin(self.depth[0], downsample=self.ds)
        rows = []
        for f in range(self.n):
            self.ctx.track_pipelined(self.P, self.refine, self.st.data_ptr(),
                                     self.depth[f + 1] if f + 1 < self.n else None)
            self.sync()
            rows.append(self.st.cpu().numpy().copy())
        return np.array(rows), rows[-1]

    def run(self, form):
        return getattr(self, form[0])(*form[1:])

    # ---- expected values (this context has no transport)
    def emulate(self, make, poses, world):
        """(script, own rows, x, winners) of the module docstring's loop."""
        import torch
        from hpe.dist import pick_best
        assert self.ctx.subswarm_info()["nranks"] == 0
        self.reset()
        script, own, xs, win = [], [], [], []
        for f in range(self.n):
            o = self._frame(f)
            sc = np.array(make(f, o, poses[f]), dtype=np.float64)
            assert sc.shape == (world, 27)
            rows = sc.copy()
            rows[self.rank] = o
            x = pick_best(torch.from_numpy(rows)).numpy().copy()
            w = [k for k in range(world) if _same(rows[k], x)][0]
            script.append(sc); own.append(o); xs.append(x); win.append(w)
            self.st.copy_(torch.from_numpy(x))
            torch.cuda.synchronize()
        return np.array(script), np.array(own), np.array(xs), win


def _assert_run(got, x, what):
    h, st = got
    assert _same(h, x), (what, np.argwhere(_bits(h) != _bits(x))[:4].tolist())
    assert _same(st, x[-1]), what


def _assert_peers_matter(own, x, win, rank):
    """A peer-wins frame's picked pose is far from the own one (a refine started from the
    wrong row lands elsewhere)."""
    peers = [f for f, w in enumerate(win) if w != rank]
    assert peers
    for f in peers:
        assert np.max(np.abs(x[f, :26] - own[f, :26])) > 1e-3, f


INF = float("inf")
# frame -> {peer: cost}; the expected winners at rank 3 of 8 beside them
SCRIPT_A = [{5: ("x", 0.5)}, {}, {1: "tie"}, {6: "tie"},
            {7: ("v", float("nan"))}, {4: ("v", -INF), 1: ("v", INF)}, {0: "tie", 2: "tie"}]
WIN_A = [5, 3, 1, 3, 3, 4, 0]
SCRIPT_B = [{}, {7: ("x", 0.25)}, {4: "tie"}, {0: "tie"}, {2: ("v", -INF)},
            {0: ("v", float("nan")), 6: ("v", INF)}, {6: ("x", 0.5)}]
WIN_B = [3, 7, 3, 0, 2, 3, 6]
GRAPH_FORMS = [("seq", 1), ("seq", 3), ("seq", 8), ("raw", 8), ("raw", 3), ("pipelined",),
               ("frame_dev",)]


def test_every_pick_event_in_every_tracking_form(np_hand):
    """World 8, rank 3, 7 frames: a peer wins, own wins, an exact tie with a lower and with a
    higher rank, a NaN peer with an attractive pose, -inf / +inf peers, a three-way tie --
    at both pick sites (chunks 3 + 3 + 1 put frames 2, 5, 6 at k_pick_best and the rest
    inside k_refine; at 8, frames 0..5 are in-refine; at 1 and in the per-frame forms every
    pick is a k_pick_best launch), through hpe_track_sequence_dev, hpe_track_raw_sequence_dev,
    hpe_track_pipelined, hpe_track_frame_dev and the direct form.  A rewound replay captures
    nothing; a second script of the same shape (other winners) is served by the same graphs:
    the script is read from the device at replay, not baked into a graph."""
    world, rank, n = 8, 3, 7
    poses, depth = _frames(np_hand, n, seed=83)
    E = Rig(depth, 32, 6, rank)
    sa, own_a, xa, win_a = E.emulate(_table_script(SCRIPT_A, world, rank), poses, world)
    sb, own_b, xb, win_b = E.emulate(_table_script(SCRIPT_B, world, rank), poses, world)
    E.close()
    assert win_a == WIN_A and win_b == WIN_B, (win_a, win_b)
    _assert_peers_matter(own_a, xa, win_a, rank)
    _assert_peers_matter(own_b, xb, win_b, rank)
    # the NaN peer's pose is attractive: the true pose's neighbour, as every peer's
    assert np.isnan(sa[4, 7, 26]) and not _same(xa, xb)

    T = Rig(depth, 32, 6, rank)
    ctx = T.ctx
    T.raw(8)  # every buffer a graph uses allocated: no later form bumps the graph epoch
    ctx.subswarm_init_scripted(sa, rank)
    info = ctx.subswarm_info()
    assert info["nranks"] == world and info["rank"] == rank and info["in_graphs"]
    for form in GRAPH_FORMS:
        c0 = ctx.graph_captures()
        _assert_run(T.run(form), xa, form)  # 7 exchanges: the counter wraps back to 0
        c1 = ctx.graph_captures()
        assert c1 > c0, form
        _assert_run(T.run(form), xa, (form, "wrapped"))
        ctx.subswarm_init_scripted(sa, rank)  # rewound
        _assert_run(T.run(form), xa, (form, "rewound"))
        assert ctx.graph_captures() == c1, form
    # a rewind in the middle of the script: 3 exchanges, then the script again from frame 0
    _assert_run(T.seq(3, n=3), xa[:3], "3 frames")
    ctx.subswarm_init_scripted(sa, rank)
    _assert_run(T.seq(3), xa, "after a rewind at exchange 3")
    # the second script, same shape: the captured graphs serve it
    c1 = ctx.graph_captures()
    ctx.subswarm_init_scripted(sb, rank)
    for form in GRAPH_FORMS:
        _assert_run(T.run(form), xb, (form, "script B"))
    assert ctx.graph_captures() == c1
    # the direct form (hpe_subswarm_enable 2): the same bits, nothing captured
    ctx.subswarm_init_scripted(sa, rank)
    ctx.subswarm_enable(True, direct=True)
    assert not ctx.subswarm_info()["in_graphs"]
    for form in (("seq", 3), ("raw", 8), ("pipelined",), ("frame_dev",)):
        _assert_run(T.run(form), xa, (form, "direct"))
    assert ctx.graph_captures() == c1
    ctx.subswarm_enable(True)
    assert ctx.subswarm_info()["in_graphs"]
    _assert_run(T.seq(8), xa, "graphs again")
    assert ctx.graph_captures() == c1
    # a script of another shape is a new transport: new graphs
    ctx.subswarm_init_scripted(np.concatenate([sa, sa[:1]]), rank)
    _assert_run(T.seq(8), xa, "8-frame script")
    assert ctx.graph_captures() > c1
    ctx.subswarm_fini()
    assert ctx.subswarm_info()["nranks"] == 0
    T.close()


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1), (64, 0), (64, 63)])
def test_rank_and_world_edges(np_hand, world, rank):
    """Worlds 1, 2 and 64 at the first and the last rank, 3 frames in one chunk: the row
    farthest from the own one wins, own wins, an exact tie with it (the lower rank wins).
    The gather buffer is NaN before the first frame; afterwards its rows != rank are the last
    script frame's, bit for bit, and row `rank` is the frame's own result.  World 1 with a
    script is the plain loop."""
    n = 3
    poses, depth = _frames(np_hand, n, seed=89)
    far = 0 if rank == world - 1 else world - 1
    table = [{far: ("x", 0.5)}, {}, {far: "tie"}] if world > 1 else [{}, {}, {}]
    E = Rig(depth, 32, 6, rank)
    sc, own, x, win = E.emulate(_table_script(table, world, rank), poses, world)
    plain = E.frame_dev()
    E.close()
    if world == 1:
        assert win == [0, 0, 0] and _same(x, own) and _same(plain[0], x)
    else:
        assert win == [far, rank, min(far, rank)], win
        _assert_peers_matter(own, x, win, rank)
    T = Rig(depth, 32, 6, rank)
    T.ctx.subswarm_init_scripted(sc, rank)
    info = T.ctx.subswarm_info(gathered=True)
    assert info["nranks"] == world and info["rank"] == rank
    assert info["gathered"].shape == (world, 27) and np.isnan(info["gathered"]).all()
    _assert_run(T.seq(8), x, "seq 8")
    g = T.ctx.subswarm_info(gathered=True)["gathered"]
    for w in range(world):
        assert _same(g[w], own[2] if w == rank else sc[2, w]), w
    _assert_run(T.raw(8), x, "raw 8")
    T.close()


FULL = dict(downsample=False)
FORMS = {  # the kernel instantiations that take the pick: env, Rig arguments
    "block-P256-staged-handframe": ({"HPE_PSO_FORM": "block"}, dict(P=256, maxiter=6, exact=False)),
    "wave2-P1024-staged-handframe": ({"HPE_PSO_FORM": "wave", "HPE_PSO_WPP": "2"},
                                     dict(P=1024, maxiter=4, exact=False)),
    "block-P32-staged-chain": ({"HPE_PSO_FORM": "block"}, dict(P=32, maxiter=6, exact=True)),
    "block-P32-full-mw-handframe": ({"HPE_PSO_FORM": "block", "HPE_REFINE_MW": "1"},
                                    dict(P=32, maxiter=6, exact=False, **FULL)),
    "block-P32-full-mw-chain": ({"HPE_PSO_FORM": "block", "HPE_REFINE_MW": "1"},
                                dict(P=32, maxiter=6, exact=True, **FULL)),
    "block-P32-full-1wg-handframe": ({"HPE_PSO_FORM": "block", "HPE_REFINE_MW": "0"},
                                     dict(P=32, maxiter=6, exact=False, **FULL)),
}


@pytest.mark.parametrize("name", list(FORMS))
def test_every_kernel_instantiation_that_takes_the_pick(np_hand, oracle, name, monkeypatch):
    """World 8, rank 3, 4 frames (peers win frames 0 and 2, own wins 1 and 3), chunks of 8
    (frames 0..2 picked inside k_refine) and 2 (frames 0, 2 inside k_refine; 1, 3 by
    k_pick_best), in fresh contexts: both generation forms (k_pso_final's gather row) and
    every refine instantiation that takes a DevPick -- staged, multi-workgroup and
    single-workgroup unstaged, hand-frame and reference chain; the raw-sequence form too
    (the refine launch that also prepares the next frame)."""
    world, rank, n = 8, 3, 4
    env, kw = FORMS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(kw)
    P, maxiter = kw.pop("P"), kw.pop("maxiter")
    poses, depth = _frames(np_hand, n, seed=97)
    if not kw.get("downsample", True):
        assert oracle.preprocess(depth[0], downsample=False).n > 2048
    # the last row wins inside k_refine (a pick over world - 1 rows would miss it); own wins
    # frames 1 and 3 through an exact tie with a higher rank (the tie rule at both sites)
    table = [{7: ("x", 0.5)}, {5: "tie"}, {0: ("x", 0.25), 5: ("x", 0.5)},
             {1: ("v", INF), 6: "tie"}]
    E = Rig(depth, P, maxiter, rank, **kw)
    sc, own, x, win = E.emulate(_table_script(table, world, rank), poses, world)
    E.close()
    assert win == [7, 3, 0, 3], win
    _assert_peers_matter(own, x, win, rank)
    T = Rig(depth, P, maxiter, rank, **kw)
    T.ctx.subswarm_init_scripted(sc, rank)
    for form in (("seq", 8), ("seq", 2), ("raw", 8)):
        _assert_run(T.run(form), x, (name, form))
    assert T.ctx.subswarm_info()["in_graphs"] and T.ctx.graph_captures() > 0
    T.close()


@pytest.mark.parametrize("peers", ["finite", "nan"])
def test_nan_worlds_through_an_empty_frame(np_hand, peers):
    """Frame 1 of 3 is all background: the own cost is NaN and bestp zeros.  With finite
    peers a peer wins and frame 2 is tracked from its pose; with every peer NaN as well the
    rule's all-NaN case picks row 0 (a peer's: this is rank 3).  Chunks of 8 (the pick inside
    frame 2's refine) and 1."""
    world, rank, n = 8, 3, 3
    poses, depth = _frames(np_hand, n, seed=101, empty=(1,))
    mid = {w: ("v", 10.0 - w) for w in range(world)} if peers == "finite" else {}
    table = [{}, mid, {}]  # frame 1's default: 2 x NaN = NaN
    E = Rig(depth, 32, 6, rank)
    sc, own, x, win = E.emulate(_table_script(table, world, rank), poses, world)
    E.close()
    assert np.isnan(own[1, 26]) and not own[1, :26].any()
    if peers == "nan":
        assert np.isnan(sc[1, [w for w in range(world) if w != rank], 26]).all()
    w1 = 7 if peers == "finite" else 0
    assert win == [rank, w1, rank], win
    assert _same(x[1], sc[1, w1]) and np.max(np.abs(x[1, :26] - own[1, :26])) > 1e-3
    T = Rig(depth, 32, 6, rank)
    T.ctx.subswarm_init_scripted(sc, rank)
    for form in (("seq", 8), ("seq", 1), ("raw", 8)):
        _assert_run(T.run(form), x, (peers, form))
    T.close()


def test_smaller_paths_and_argument_errors(np_hand):
    """refine = 0 (no refine launch: every pick is a k_pick_best launch); d_hist = NULL (the
    final state alone); the exchange suspended while a script is loaded (the plain loop's
    bits; the exchange counter rests) and resumed; the entry's argument errors on a live
    context; fini and re-initialisation."""
    import hpe
    E_ARG, E_STATE = hpe._lib.HPE_E_ARG, hpe._lib.HPE_E_STATE
    world, rank, n = 8, 3, 4
    poses, depth = _frames(np_hand, n, seed=103)
    table = [{2: ("x", 0.5)}, {7: "tie"}, {0: "tie"}, {4: ("x", 0.5)}]
    make = _table_script(table, world, rank)
    E0 = Rig(depth, 32, 6, rank, refine=0)
    sc0, own0, x0, win0 = E0.emulate(make, poses, world)
    E0.close()
    E = Rig(depth, 32, 6, rank)
    sc, own, x, win = E.emulate(make, poses, world)
    plain = E.frame_dev()
    E.close()
    assert win0 == [2, 3, 0, 4] and win == win0
    _assert_peers_matter(own0, x0, win0, rank)
    _assert_peers_matter(own, x, win, rank)
    T0 = Rig(depth, 32, 6, rank, refine=0)
    T0.ctx.subswarm_init_scripted(sc0, rank)
    for form in (("seq", 8), ("seq", 3), ("raw", 8)):
        _assert_run(T0.run(form), x0, ("refine 0", form))
    T0.close()

    T = Rig(depth, 32, 6, rank)
    ctx, lib = T.ctx, T.ctx.lib
    assert lib.hpe_subswarm_enable(ctx.h, 1) == E_STATE  # no transport yet
    p = sc.ctypes.data_as(hpe._lib.dp)
    for nranks, r, s, frames in ((0, 0, p, n), (65, 0, p, n), (8, 8, p, n), (8, -1, p, n),
                                 (8, 3, p, 0), (8, 3, p, -1), (8, 3, None, n)):
        assert lib.hpe_subswarm_init_scripted(ctx.h, nranks, r, s, frames) == E_ARG
    assert ctx.subswarm_info()["nranks"] == 0  # a refused call sets no transport
    ctx.subswarm_init_scripted(sc, rank)
    for K in (8, 3):  # no history: the final state alone
        h, st = T.seq(K, hist=False)
        assert _same(st, x[-1]) and (h == SENTINEL).all(), K
    ctx.subswarm_enable(False)  # suspended: the plain loop
    _assert_run(T.seq(3), plain[0], "suspended")
    ctx.subswarm_enable(True)  # resumed: the counter rested at 0 (two 4-frame runs wrapped)
    _assert_run(T.seq(3), x, "resumed")
    ctx.subswarm_init_scripted(sc[:, :2], 1)  # another world replaces the transport
    assert ctx.subswarm_info()["nranks"] == 2 and ctx.subswarm_info()["rank"] == 1
    ctx.subswarm_fini()
    assert ctx.subswarm_info()["nranks"] == 0
    _assert_run(T.seq(3), plain[0], "after fini")
    T.close()


# ---------------------------------------------------------------- the CPU-oracle anchor
ANCHOR_SEED = 71  # chosen on the CPU oracle alone: ranks 2, 5, 4, 6, 1, 5 win; margins >= 7e-2


@pytest.fixture(scope="module")
def anchor(oracle, ora_hand, np_hand):
    """Config 5's shape (world 8, P = 1024, seeds 1000..1007; maxiter 11) on 6 frames, the
    oracle's eight subswarms free-running: refine, pso_evolve(seed = 1000 + r), cal_cost, the
    best of 8, the next frame from the winner."""
    world, P, maxiter, n = 8, 1024, 11, 6
    poses, depth = _frames(np_hand, n, seed=ANCHOR_SEED)
    ub, lb, sd = oracle_np.reference_bounds()
    x = oracle_np.X0.copy()
    rows, best, win = [], [], []
    for f in range(n):
        obs = oracle.preprocess(depth[f])
        xr, _ = oracle.refine(ora_hand, obs, x, rigid=REFINE_RIGID)
        fr = []
        for r in range(world):
            b, _, _ = oracle.pso_evolve(ora_hand, obs, xr, P, maxiter, lb, ub, sd, seed=1000 + r)
            fr.append(np.concatenate([b, [oracle.cal_cost(ora_hand, obs, b)]]))
        fr = np.array(fr)
        c = np.sort(fr[:, 26])
        # rounding cannot flip a winner: best and second best differ by > 100 COST_RTOL
        assert (c[1] - c[0]) > 100 * COST_RTOL * abs(c[0]), (f, c[:2])
        w = int(np.argmin(fr[:, 26]))
        rows.append(fr); best.append(fr[w]); win.append(w)
        x = fr[w, :26].copy()
    assert len(set(win)) >= 2, win
    return dict(poses=poses, depth=depth, rows=np.array(rows), best=np.array(best), win=win,
                P=P, maxiter=maxiter, world=world)


@pytest.mark.parametrize("rank", [0, 5])
def test_anchor_against_the_cpu_oracle(anchor, rank):
    """The GPU as rank r of 8 with the oracle's rows as the script: its history equals the
    oracle's best-of-8 history within POSE_TOL / COST_RTOL, bit-equals the script row on the
    frames a peer wins, and bit-equals the emulation throughout."""
    a = anchor
    E = Rig(a["depth"], a["P"], a["maxiter"], rank)
    sc, own, x, win = E.emulate(lambda f, o, t: a["rows"][f], a["poses"], a["world"])
    E.close()
    assert win == a["win"], (win, a["win"])
    T = Rig(a["depth"], a["P"], a["maxiter"], rank)
    T.ctx.subswarm_init_scripted(sc, rank)
    for form in (("raw", 8), ("seq", 3)):
        h, st = T.run(form)
        _assert_run((h, st), x, form)
        np.testing.assert_allclose(h[:, :26], a["best"][:, :26], rtol=0, atol=POSE_TOL)
        assert (np.abs(h[:, 26] - a["best"][:, 26]) <= COST_RTOL * np.abs(a["best"][:, 26])).all()
        for f, w in enumerate(win):
            if w != rank:
                assert _same(h[f], sc[f, w]), (form, f)
    T.close()
