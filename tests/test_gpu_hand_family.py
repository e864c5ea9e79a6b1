"""The hand family (hand_data.hand_family) on the GPU against the oracles: every piece that reads
the hand constants (DevHand), on hands that are not the reference subject's.

One context per family hand, created when first needed, shared by the file and closed at its
end.  The yardstick is always the C oracle with the same hand (oracle.hand(geo, rad, cmc,
spacing)), never another GPU run; frames are rendered by oracle_np.render_depth_mm with the same
hand's numpy model, so the tracker sees a hand of its own size.  Tolerances are those of
tests/test_gpu_parity.py: FK and joints 1e-9 cm, costs relative 1e-9 and matches through its
tie-aware comparator, pso_evolve / refine / tracking poses 1e-6 and costs relative 1e-8,
pso_optimise poses 1e-5 and costs relative 1e-7.

The lane tests put the family into the lane table of ONE context created with `ref`
(hpe_set_batch_hands) and compare lane b with the oracle's loop under hand b: equal hands sit
at unequal lane indices, so a lane that read another lane's entry -- in every kernel form alike
-- would show.

Small shapes: 250-point clouds (full resolution once for V and uneven), P <= 32 outside the one
ragged wave case, at most 3 frames.  Every test prints the differences it measured.
"""
import numpy as np
import pytest

import hand_data
from hand_data import REFINE_RIGID
import oracle_np
from test_gpu_parity import _match_equiv, _refine_form

pytestmark = pytest.mark.gpu

FAMILY = hand_data.FAMILY
FOCAL = 241.42
W, C1, C2 = 0.7298, 1.49618, 1.49618
TIE = 1e-13         # tests/test_gpu_configs.py TIE_MARGIN
CLEAR = 1e-12       # a refine whose smallest decision margin reaches this must count as the oracle
LANES4 = ("uneven", "ref", "small", "V")
LANES16 = FAMILY + ("zero_sp", "V", "right_angle", "ref", "mirror", "large", "uneven", "small")
LANE_P, LANE_MAXITER, LANE_NF, LANE_K = 32, 4, 3, 2
SENTINEL = -7.0


class Pool:
    def __init__(self, oracle):
        self.oracle = oracle
        self.family = hand_data.hand_family()
        self.hands, self.waves, self.oras = {}, {}, {}
        self.frames, self.seeds, self.loops, self.opts = {}, {}, {}, {}
        self.slots, self.next_slot = {}, 16

    # ---- the hands
    def hand(self, name):
        if name not in self.hands:
            self.hands[name] = hand_data.family_gpu_hand(self.family[name])
        return self.hands[name]

    def wave_hand(self, name, wpp, monkeypatch):
        """A further context of hand `name` created under HPE_PSO_FORM=wave, HPE_PSO_WPP=wpp."""
        if (name, wpp) not in self.waves:
            monkeypatch.setenv("HPE_PSO_FORM", "wave")
            monkeypatch.setenv("HPE_PSO_WPP", str(wpp))
            self.waves[(name, wpp)] = hand_data.family_gpu_hand(self.family[name])
        return self.waves[(name, wpp)]

    def ora(self, name):
        """(C oracle hand, numpy hand)"""
        if name not in self.oras:
            self.oras[name] = hand_data.family_oracle_hands(self.oracle, self.family[name])
        return self.oras[name]

    def params(self, names):
        return [hand_data.family_gpu_hand(self.family[n], params_only=True) for n in names]

    def close(self):
        for h in list(self.hands.values()) + list(self.waves.values()):
            h.ctx.close()

    # ---- frames, rendered once per (hand, trajectory, frame) by the hand's numpy model
    def frame(self, name, n, seed, k):
        key = (name, n, seed, k)
        if key not in self.frames:
            th = hand_data.trajectory(n, seed=seed)[k]
            self.frames[key] = oracle_np.render_depth_mm(self.ora(name)[1], th)
        return self.frames[key]

    def obs_pair(self, name, depth_mm, downsample=True):
        import hpe
        obs = self.oracle.preprocess(depth_mm, downsample=downsample)
        om = hpe.observedmodel()
        om.to_cm, om.downsample, om.focal_len = True, downsample, FOCAL
        om.set_depth_mm(depth_mm)
        return obs, om

    def pso(self, maxiter, ctx=None):
        import hpe
        ub, lb, sd = oracle_np.reference_bounds()
        pso = hpe.PSO()
        pso.set_pso_params(ub, lb, sd, W, C1, C2, maxiter, 1e-8, 1e-8)
        if ctx is not None:
            pso._push(ctx)
        return pso

    # ---- the refine's seed: the clearest decisions among trajectory(2, seed=0..15)[1]
    def refine_seed(self, name, rigid):
        if (name, rigid) not in self.seeds:
            best = (-1.0, None)
            for s in range(16):
                obs = self.oracle.preprocess(self.frame(name, 2, s, 1))
                _, _, m = self.oracle.refine_log(self.ora(name)[0], obs, oracle_np.X0, rigid=rigid)
                best = max(best, (float(m.min()), s))
            self.seeds[(name, rigid)] = best
        return self.seeds[(name, rigid)]

    # ---- the oracle's tracking loop (testmodel.cpp:117-139) under a hand, once per stream
    def loop(self, name, seed, P, maxiter, nf=LANE_NF):
        key = (name, seed, P, maxiter, nf)
        if key not in self.loops:
            o, ora = self.oracle, self.ora(name)[0]
            ub, lb, sd = oracle_np.reference_bounds()
            x, out = oracle_np.X0.copy(), []
            for f in range(nf):
                obs = o.preprocess(self.frame(name, nf, seed, f))
                x, _ = o.refine(ora, obs, x, rigid=REFINE_RIGID)
                x, _, _ = o.pso_evolve(ora, obs, x, P, maxiter, lb, ub, sd)
                out.append(np.append(x, o.cal_cost(ora, obs, x)))
            self.loops[key] = np.array(out)
        return self.loops[key]

    def optimise(self, name, P, maxiter):
        """oracle.pso_optimise under hand `name` on its frame of trajectory(2, seed=21)[1]."""
        key = (name, P, maxiter)
        if key not in self.opts:
            ub, lb, sd = oracle_np.reference_bounds()
            obs = self.oracle.preprocess(self.frame(name, 2, 21, 1))
            self.opts[key] = self.oracle.pso_optimise(self.ora(name)[0], obs, oracle_np.X0.copy(), P,
                                                      maxiter, lb, ub, sd, W, C1, C2, seed=1000)
        return self.opts[key]

    def slot0(self, ctx, key, frames):
        """The frames device-prepared into consecutive slots of the batch context, once."""
        if key not in self.slots:
            self.slots[key] = self.next_slot
            for f, d in enumerate(frames):
                ctx.prepare_frame(self.next_slot + f, d)
            self.next_slot += len(frames)
            ctx.check(ctx.lib.hpe_sync(ctx.h))
        return self.slots[key]


@pytest.fixture(scope="module")
def pool(oracle):
    p = Pool(oracle)
    yield p
    p.close()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


# ---- FK
@pytest.mark.parametrize("name", FAMILY)
def test_fk_spheres_and_joints(pool, oracle, name):
    th = hand_data.family_poses()
    S, J = pool.hand(name).build_batch(th)
    Sr, Jr = zip(*[oracle.build(pool.ora(name)[0], t, joints=True) for t in th])
    ds, dj = np.abs(S - np.array(Sr)).max(), np.abs(J - np.array(Jr)).max()
    print(f"hand {name}: FK spheres {ds:.3g} cm, joints {dj:.3g} cm over {len(th)} poses")
    assert np.isfinite(S).all() and np.isfinite(J).all()
    assert ds <= 1e-9 and dj <= 1e-9


# ---- cost terms
@pytest.mark.parametrize("name,downsample", [(n, True) for n in FAMILY] +
                         [("V", False), ("uneven", False)])
def test_costs_terms_and_matches(pool, oracle, name, downsample):
    import hpe
    ora, hand = pool.ora(name)[0], pool.hand(name)
    truth = hand_data.trajectory(3, seed=5)[2]
    obs, om = pool.obs_pair(name, pool.frame(name, 3, 5, 2), downsample)
    assert (obs.n == 250) if downsample else (obs.n > 2048)
    cf = hpe.costfunc(hand, om)
    th = hand_data.random_thetas(np.random.default_rng(31), 12, x0=truth, spread=0.4)
    th[0] = truth
    cost, match = cf.cal_cost_batch(th, return_match=True)
    cost_c = cf.cal_cost_batch(th, with_collision=True)
    ref = oracle.eval_costs(ora, obs, th)
    ref_c = oracle.eval_costs(ora, obs, th, with_collision=True)
    moved, worst_t, terms = 0, 0.0, []
    for i in range(len(th)):
        S = oracle.build(ora, th[i])
        mr = oracle.correspondences(obs, S)
        moved += int((match[i] != mr).sum())
        assert _match_equiv(obs, S, match[i], mr), i
        m = np.zeros(obs.n, dtype=np.int32)
        c = cf.cal_cost2(th[i], m, True)
        cr, tr, mr2 = oracle.terms(ora, obs, th[i])
        assert _match_equiv(obs, S, m, mr2), i
        terms.append((c, cf.last_terms.copy(), cr, tr))
        worst_t = max(worst_t, abs(c - cr) / abs(cr),
                      float(np.max(np.abs(cf.last_terms - tr) / np.maximum(np.abs(tr), 1e-300))))
    print(f"hand {name} (N = {obs.n}): costs {_rel(cost, ref):.3g}, with collision "
          f"{_rel(cost_c, ref_c):.3g}, cal_cost2 terms {worst_t:.3g} (relative); "
          f"{moved} equidistant matches differ")
    np.testing.assert_allclose(cost, ref, rtol=1e-9, atol=0)
    np.testing.assert_allclose(cost_c, ref_c, rtol=1e-9, atol=0)
    for c, t, cr, tr in terms:
        assert abs(c - cr) <= 1e-9 * abs(cr)
        np.testing.assert_allclose(t, tr, rtol=1e-9, atol=1e-300)
    assert (ref_c >= ref).all()


# ---- refine_init_pose, both forms
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", FAMILY)
def test_refine_init_pose(pool, oracle, name, exact):
    import hpe
    ora, hand = pool.ora(name)[0], pool.hand(name)
    margin, seed = pool.refine_seed(name, not exact)
    obs, om = pool.obs_pair(name, pool.frame(name, 2, seed, 1))
    cf = hpe.costfunc(hand, om)
    x0 = oracle_np.X0.copy()
    with _refine_form(hand.ctx, exact) as rigid:
        assert rigid == (not exact)
        x_ref, ev_ref = oracle.refine(ora, obs, x0, rigid=rigid)
        pso = hpe.PSO()
        x = x0.copy()
        pso.refine_init_pose(x, cf)
    ev = pso.last_refine_evals
    print(f"hand {name}, {'chain' if exact else 'hand-frame'} refine: seed {seed}, smallest "
          f"decision margin {margin:.3g}; evaluations {ev} (oracle {ev_ref}), pose "
          f"{np.abs(x - x_ref).max():.3g}")
    if margin >= CLEAR:
        assert ev == ev_ref
    elif ev != ev_ref:
        flips = hand_data.tie_replay(oracle, ora, obs, x0, ev, rigid, TIE, pose=x)
        assert flips is not None, "no near-tie explains the evaluation count"
        print(f"  near-ties flipped (decision, margin): {flips}")
    np.testing.assert_allclose(x, x_ref, rtol=0, atol=1e-6)
    assert np.abs(x - x0).max() > 1e-3  # the refine moved


# ---- pso_evolve, the workgroup form and the wave form
def _check_evolve(pool, oracle, name, hand, P, maxiter, what):
    import hpe
    ora = pool.ora(name)[0]
    obs, om = pool.obs_pair(name, pool.frame(name, 2, 9, 1))
    cf = hpe.costfunc(hand, om)
    ub, lb, sd = oracle_np.reference_bounds()
    pso = pool.pso(maxiter)
    bestp, x0 = np.zeros(26), oracle_np.X0.copy()
    assert pso.pso_evolve(cf, x0, P, bestp) == 1
    rb, rc, tr = oracle.pso_evolve(ora, obs, x0, P, maxiter, lb, ub, sd, seed=1000)
    g, cnt, topo = pso.trace(cf)
    print(f"hand {name}, pso_evolve {what} P={P} maxiter={maxiter}: bestp "
          f"{np.abs(bestp - rb).max():.3g}, cost {abs(pso.last_gbest_cost - rc) / abs(rc):.3g}, "
          f"gbest trace {_rel(g, tr['gbest']):.3g}")
    np.testing.assert_allclose(bestp, rb, rtol=0, atol=1e-6)
    assert abs(pso.last_gbest_cost - rc) <= 1e-8 * abs(rc)
    np.testing.assert_allclose(g, tr["gbest"], rtol=1e-8)
    assert np.array_equal(cnt, tr["count"]) and np.array_equal(topo, tr["topo"])


@pytest.mark.parametrize("P,maxiter", [(32, 6), (7, 4)])
@pytest.mark.parametrize("name", FAMILY)
def test_pso_evolve(pool, oracle, name, P, maxiter):
    _check_evolve(pool, oracle, name, pool.hand(name), P, maxiter, "workgroup form")


@pytest.mark.parametrize("P,maxiter", [(32, 6), (1030, 3)])
@pytest.mark.parametrize("wpp", [1, 2])
@pytest.mark.parametrize("name", ["V", "uneven"])
def test_pso_evolve_wave_form(pool, oracle, name, wpp, P, maxiter, monkeypatch):
    hand = pool.wave_hand(name, wpp, monkeypatch)
    _check_evolve(pool, oracle, name, hand, P, maxiter, f"wave form, {wpp} per particle,")


# ---- pso_optimise
@pytest.mark.parametrize("name", ["V", "uneven", "mirror", "right_angle"])
def test_pso_optimise(pool, oracle, name):
    import hpe
    P, maxiter = 5, 3
    hand = pool.hand(name)
    _, om = pool.obs_pair(name, pool.frame(name, 2, 21, 1))
    cf = hpe.costfunc(hand, om)
    pso = pool.pso(maxiter)
    bestp = np.zeros(26)
    assert pso.pso_optimise(cf, oracle_np.X0.copy(), P, bestp) == 1
    rb, rc, tr = pool.optimise(name, P, maxiter)
    print(f"hand {name}, pso_optimise: bestp {np.abs(bestp - rb).max():.3g}, cost "
          f"{abs(pso.last_gbest_cost - rc) / abs(rc):.3g}, trace "
          f"{_rel(pso.last_optimise_trace, tr):.3g}")
    np.testing.assert_allclose(bestp, rb, rtol=0, atol=1e-5)
    assert abs(pso.last_gbest_cost - rc) <= 1e-7 * abs(rc)
    np.testing.assert_allclose(pso.last_optimise_trace, tr, rtol=1e-7)


# ---- tracking
@pytest.mark.parametrize("name", ["V", "small", "large", "uneven"])
def test_pipelined_tracking(pool, oracle, name):
    import torch
    P, maxiter, nf, seed = 32, 6, 3, 19
    ctx = pool.hand(name).ctx
    pool.pso(maxiter, ctx)
    depth = [pool.frame(name, nf, seed, f) for f in range(nf)]
    want = pool.loop(name, seed, P, maxiter, nf)
    st = torch.zeros(27, dtype=torch.float64, device="cuda:0")
    st[:26] = torch.from_numpy(oracle_np.X0)
    torch.cuda.synchronize()
    ctx.pipeline_begin(depth[0])
    got = []
    for f in range(nf):
        ctx.track_pipelined(P, 1, st.data_ptr(), depth[f + 1] if f + 1 < nf else None)
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        got.append(st.cpu().numpy().copy())
    got = np.array(got)
    print(f"hand {name}, pipelined tracking of {nf} frames: pose "
          f"{np.abs(got[:, :26] - want[:, :26]).max():.3g}, cost {_rel(got[:, 26], want[:, 26]):.3g}")
    np.testing.assert_allclose(got[:, :26], want[:, :26], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, 26], want[:, 26], rtol=1e-8, atol=0)


# ---- lanes against the oracle directly
def _lane_streams(names):
    """(hand, trajectory seed) of every lane: a hand's second lane tracks another stream."""
    seen, out = {}, []
    for n in names:
        out.append((n, 40 + FAMILY.index(n) + 8 * seen.get(n, 0)))
        seen[n] = seen.get(n, 0) + 1
    return out


def _check_lanes(pool, streams, hist, what):
    dp = dc = 0.0
    for b, (name, seed) in enumerate(streams):
        want = pool.loop(name, seed, LANE_P, LANE_MAXITER)
        dp = max(dp, np.abs(hist[b][:, :26] - want[:, :26]).max())
        dc = max(dc, _rel(hist[b][:, 26], want[:, 26]))
    print(f"{what}, {len(streams)} lanes: pose {dp:.3g}, cost {dc:.3g} against each lane's oracle loop")
    for b, (name, seed) in enumerate(streams):
        want = pool.loop(name, seed, LANE_P, LANE_MAXITER)
        np.testing.assert_allclose(hist[b][:, :26], want[:, :26], rtol=0, atol=1e-6,
                                   err_msg=f"lane {b} ({name})")
        np.testing.assert_allclose(hist[b][:, 26], want[:, 26], rtol=1e-8, atol=0,
                                   err_msg=f"lane {b} ({name})")


def _check_joints(pool, oracle, names, poses, joints, what):
    """joints[b][f] against oracle.build(hand_b, poses[b][f], joints=True): 1e-9 cm."""
    worst = 0.0
    for b, name in enumerate(names):
        for f in range(len(poses[b])):
            _, Jr = oracle.build(pool.ora(name)[0], poses[b][f][:26], joints=True)
            worst = max(worst, np.abs(joints[b][f] - Jr).max())
    print(f"{what}: joints {worst:.3g} cm against the oracle under each lane's hand")
    assert worst <= 1e-9


@pytest.fixture()
def batch(pool):
    """The context under test: the one created with `ref`; its lane hands are cleared after."""
    import hpe
    ctx = pool.hand("ref").ctx
    pool.pso(LANE_MAXITER, ctx)
    yield ctx
    ctx.set_batch_form("auto")
    for undo in (lambda: ctx.set_batch_report(0), lambda: ctx.set_batch_hands(None)):
        try:
            undo()
        except hpe.HpeError:
            pass  # a live batch that a failed test left behind keeps its settings


@pytest.mark.parametrize("form", ["auto", "wave"])
@pytest.mark.parametrize("names", [LANES4, LANES16], ids=["B4", "B16"])
def test_lanes_prepared(pool, oracle, batch, names, form):
    import torch
    ctx, B, n = batch, len(names), LANE_NF
    streams = _lane_streams(names)
    assert len(set(streams)) == B
    first = [pool.slot0(ctx, s, [pool.frame(s[0], n, s[1], f) for f in range(n)]) for s in streams]
    st = torch.zeros((B, 27), dtype=torch.float64, device="cuda:0")
    st[:, :26] = torch.from_numpy(oracle_np.X0)
    hist = torch.full((B, n, 27), SENTINEL, dtype=torch.float64, device="cuda:0")
    J = torch.full((B, n, 21, 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.set_batch_hands(pool.params(names))
    ctx.set_batch_form(form)
    ctx.track_batch(LANE_P, 1, st.data_ptr(), first, n, LANE_K, hist.data_ptr())
    ctx.lane_joints(B, n, hist.data_ptr(), J.data_ptr(), None)
    ctx.check(ctx.lib.hpe_sync(ctx.h))
    h, j = hist.cpu().numpy(), J.cpu().numpy()
    assert np.isfinite(h).all() and np.array_equal(st.cpu().numpy(), h[:, -1])
    _check_lanes(pool, streams, h, f"prepared batch, form {form}")
    _check_joints(pool, oracle, names, h, j, f"hpe_lane_joints_dev over the history, form {form}")
    if form == "auto" and B == 4:
        # a constructed pair: equal poses under different hands report different joints
        hist[:] = 0.0
        hist[:, :, :26] = torch.from_numpy(oracle_np.X0)
        torch.cuda.synchronize()
        ctx.lane_joints(B, n, hist.data_ptr(), J.data_ptr(), None)
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        j0 = J.cpu().numpy()
        _check_joints(pool, oracle, names, hist.cpu().numpy(), j0, "equal poses in every lane")
        for a in range(B):
            for b in range(a + 1, B):
                assert np.abs(j0[a] - j0[b]).max() > 0.1, (names[a], names[b])


def test_lanes_live_with_reports(pool, oracle, batch):
    import torch
    names = LANES16
    ctx, B, n = batch, len(names), LANE_NF
    streams = _lane_streams(names)
    fr = [[pool.frame(s[0], n, s[1], f) for f in range(n)] for s in streams]
    st = torch.zeros((B, 27), dtype=torch.float64, device="cuda:0")
    st[:, :26] = torch.from_numpy(oracle_np.X0)
    torch.cuda.synchronize()
    ctx.set_batch_hands(pool.params(names))
    ctx.set_batch_report(4)
    ctx.batch_pipeline_begin([x[0] for x in fr])
    states, reports = [], []
    for f in range(n):
        ctx.track_batch_pipelined(LANE_P, 1, st.data_ptr(), [x[f + 1] for x in fr] if f + 1 < n else None)
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        states.append(st.cpu().numpy().copy())
        reports.append([ctx.batch_report(b) for b in range(B)])
    hist = np.array(states).transpose(1, 0, 2)  # B x n x 27
    assert np.isfinite(hist).all()
    _check_lanes(pool, streams, hist, "live batch")
    for f in range(n):
        for b in range(B):
            r = reports[f][b]
            assert (r.seq, r.lane) == (f + 1, b)
            assert np.array_equal(r.state, hist[b, f])
    joints = [[reports[f][b].joints for f in range(n)] for b in range(B)]
    _check_joints(pool, oracle, names, hist, joints, "live batch reports")


def test_pso_optimise_batch(pool, oracle, batch):
    import torch
    names, P, maxiter = ("V", "mirror", "right_angle", "ref"), 5, 3
    ctx, B = batch, 4
    pool.pso(maxiter, ctx)
    slots = [pool.slot0(ctx, ("opt", nm), [pool.frame(nm, 2, 21, 1)]) for nm in names]
    st = torch.zeros((B, 27), dtype=torch.float64, device="cuda:0")
    st[:, :26] = torch.from_numpy(oracle_np.X0)
    tr = torch.full((B, maxiter - 1), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.set_batch_hands(pool.params(names))
    ctx.pso_optimise_batch(P, st.data_ptr(), slots, tr.data_ptr())
    ctx.check(ctx.lib.hpe_sync(ctx.h))
    got, trace = st.cpu().numpy(), tr.cpu().numpy()
    want = [pool.optimise(nm, P, maxiter) for nm in names]
    for b, nm in enumerate(names):
        rb, rc, rt = want[b]
        print(f"lane {b} ({nm}), pso_optimise_batch: bestp {np.abs(got[b, :26] - rb).max():.3g}, "
              f"cost {abs(got[b, 26] - rc) / abs(rc):.3g}, trace {_rel(trace[b], rt):.3g}")
    for b, nm in enumerate(names):
        rb, rc, rt = want[b]
        np.testing.assert_allclose(got[b, :26], rb, rtol=0, atol=1e-5, err_msg=nm)
        assert abs(got[b, 26] - rc) <= 1e-7 * abs(rc), nm
        np.testing.assert_allclose(trace[b], rt, rtol=1e-7, err_msg=nm)
    # the lanes' hands matter: no two oracle results are alike
    for a in range(B):
        for b in range(a + 1, B):
            assert abs(want[a][1] - want[b][1]) > 1e-6 * abs(want[a][1])


# ---- renderer
@pytest.mark.parametrize("name", FAMILY)
def test_render_matches_numpy(pool, name):
    ctx, nph = pool.hand(name).ctx, pool.ora(name)[1]
    poses = [oracle_np.X0] + list(hand_data.trajectory(3, seed=5)[1:])
    worst_m, worst_d = 1.0, 0.0
    for k, th in enumerate(poses):
        d_gpu = ctx.render_depth(th)
        d_np = oracle_np.render_depth_mm(nph, th) if k == 0 else pool.frame(name, 3, 5, k)
        both = (d_gpu > 0) & (d_np > 0)
        worst_m = min(worst_m, ((d_gpu > 0) == (d_np > 0)).mean())
        worst_d = max(worst_d, np.abs(d_gpu[both] - d_np[both]).max())
        assert both.sum() > 1000
    print(f"hand {name}, renderer: mask agreement {worst_m:.6f}, depth {worst_d:.3g} mm")
    assert worst_m > 0.9995
    assert worst_d < 1e-3
