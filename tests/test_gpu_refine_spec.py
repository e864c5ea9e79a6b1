"""The speculated translation block of the staged refine (k_refine<..., SPEC>):
a second workgroup runs refine_init_pose's translation block from the pose of every
rotation-block line search while that search runs, and the leader takes its result when the
rotation block ends on a failing search.  The claim is exactness: with the speculation on, the
pose (compared as bits) and the evaluation count are those of the one-workgroup form -- on
single calls whose rotation block ends either way, through captured and replayed tracking
graphs (a commit or a result of one launch must never be seen by the next), with the leader's
wait for the result cut to zero polls (the bounded fallback), and across changes of the switch.

All frames are N = 250 clouds: down-sampled synthetic frames of the seed-0 trajectory."""
import ctypes as C

import numpy as np
import pytest

import hand_data
from hand_data import REFINE_RIGID
import oracle_np

pytestmark = pytest.mark.gpu

# single calls: (frame of the trajectory, start pose).  "truth": the previous frame's true pose;
# "tracked": the pose the oracle's own tracking (32 particles, 3 generations) reached on the
# previous frame.  Chosen with the oracle: 10, 12, 23 end the rotation block on tol / iter (the
# abort path), 20 and the tracked ones on a failing search (the commit path); every decision of
# these refines has a relative margin above 5e-11, far from the 1e-13 near-tie floor, so the
# evaluation counts equal the oracle's.
TRUTH_FRAMES = (10, 12, 23, 20)
TRACKED_FRAMES = (2, 3)
P, MAXITER = 32, 4
N_SEQ, K_GRAPH, N_PIPE = 16, 8, 4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rotation_block_failed(oracle, ora_hand, obs, x0):
    """(the oracle's refined pose, its evaluations, whether its rotation block ended on a failing
    line search) from the oracle's log of the Goldstein searches.  A block ends at its first
    failing search, and the translation block always runs at least one search: the rotation
    block failed iff two searches failed, or one that is not the call's last."""
    lib = oracle.lib
    lib.ora_set_gold_log.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    lib.ora_gold_log_count.restype = C.c_int
    buf = np.zeros(128, dtype=np.uint64)
    lib.ora_set_gold_log(buf.ctypes.data_as(C.POINTER(C.c_uint64)), len(buf))
    try:
        x, ev = oracle.refine(ora_hand, obs, x0, rigid=REFINE_RIGID)
        n = lib.ora_gold_log_count()
    finally:
        lib.ora_set_gold_log(C.POINTER(C.c_uint64)(), 0)
    assert n <= len(buf)
    fails = [i for i in range(n) if not (int(buf[i]) >> 40) & 1]
    return x, ev, len(fails) == 2 or (len(fails) == 1 and fails[0] != n - 1)


@pytest.fixture(scope="module")
def depth(np_hand):
    poses = hand_data.trajectory(max(TRUTH_FRAMES) + 1, seed=0, revert=0.02)
    return poses, {f: oracle_np.render_depth_mm(np_hand, poses[f])
                   for f in sorted(set(TRUTH_FRAMES) | set(range(N_SEQ + 1)))}


@pytest.fixture(scope="module")
def cases(oracle, ora_hand, depth):
    """The single calls, judged on the CPU: [(depth, x0, oracle pose, oracle evals, failed)]."""
    poses, dm = depth
    ub, lb, sd = oracle_np.reference_bounds()
    starts = [(f, poses[f - 1]) for f in TRUTH_FRAMES]
    x = poses[0].copy()
    for f in range(1, max(TRACKED_FRAMES) + 1):
        obs = oracle.preprocess(dm[f], downsample=True)
        if f in TRACKED_FRAMES:
            starts.append((f, x.copy()))
        x, _ = oracle.refine(ora_hand, obs, x, rigid=REFINE_RIGID)
        x, _, _ = oracle.pso_evolve(ora_hand, obs, x, 32, 3, lb, ub, sd, seed=1000)
    out = []
    for f, x0 in starts:
        obs = oracle.preprocess(dm[f], downsample=True)
        assert obs.n == 250
        xr, ev, failed = _rotation_block_failed(oracle, ora_hand, obs, x0)
        out.append((dm[f], x0, xr, ev, failed))
    # both ends of the rotation block are among the frames before the GPU is trusted
    assert sum(1 for c in out if c[4]) >= 2 and sum(1 for c in out if not c[4]) >= 2
    return out


@pytest.fixture(scope="module")
def gh():
    import hpe
    return hpe.reference_hand(device=0)


def _refine_all(hand, cases, spec):
    """[(pose, evals)] of hpe_refine_init_pose on every case with the speculation on / off."""
    import hpe
    was = hand.ctx.refine_spec
    hand.ctx.refine_spec = spec
    out = []
    try:
        for d, x0, _, _, _ in cases:
            om = hpe.observedmodel()
            om.to_cm, om.downsample, om.focal_len = True, True, 241.42
            om.set_depth_mm(d)
            cf = hpe.costfunc(hand, om)
            pso = hpe.PSO()
            x = x0.copy()
            pso.refine_init_pose(x, cf)
            out.append((x, pso.last_refine_evals))
    finally:
        hand.ctx.refine_spec = was
    return out


@pytest.fixture(scope="module")
def single_on(gh, cases):
    assert gh.ctx.refine_spec  # on by default
    return _refine_all(gh, cases, True)


def test_single_calls_bitwise(gh, cases, single_on):
    off = _refine_all(gh, cases, False)
    for k, ((xa, ea), (xb, eb), (_, _, xr, ev, failed)) in enumerate(zip(single_on, off, cases)):
        print(f"case {k}: rotation block {'failed' if failed else 'tol/iter'}, evals on {ea} "
              f"off {eb} oracle {ev}, max |on - off| {np.max(np.abs(xa - xb)):.3e}")
        assert np.array_equal(_bits(xa), _bits(xb)), k
        assert ea == eb == ev, k
        np.testing.assert_allclose(xa, xr, rtol=0, atol=1e-6)


def test_bounded_fallback(cases, single_on, monkeypatch):
    """HPE_SPEC_SPIN=0 (read at hpe_create): the leader's wait for a committed result has no
    polls, so it aborts the runner and runs the translation block itself -- the same bits, and
    nothing flagged."""
    import hpe
    monkeypatch.setenv("HPE_SPEC_SPIN", "0")
    hand = hpe.reference_hand(device=0)
    monkeypatch.delenv("HPE_SPEC_SPIN")
    assert hand.ctx.refine_spec
    got = _refine_all(hand, cases, True)
    assert hand.ctx.lib.hpe_sync(hand.ctx.h) == 0
    for k, ((xa, ea), (xb, eb)) in enumerate(zip(got, single_on)):
        assert np.array_equal(_bits(xa), _bits(xb)), k
        assert ea == eb, k
    hand.ctx.close()


def _push_params(ctx):
    import hpe
    ub, lb, sd = oracle_np.reference_bounds()
    pso = hpe.PSO()
    pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
    pso._push(ctx)


def _sequence(ctx, d_raw, bufs):
    """One pass of hpe_track_raw_sequence_dev over N_SEQ frames: the (N_SEQ, 27) history."""
    import torch
    st, hist = bufs
    st[:26] = torch.from_numpy(oracle_np.X0)
    st[26] = 0.0
    hist.fill_(float("nan"))
    torch.cuda.synchronize()
    ctx.track_raw_sequence(P, 1, st.data_ptr(), d_raw.data_ptr(), N_SEQ, frames_per_graph=K_GRAPH,
                           d_hist_ptr=hist.data_ptr())
    ctx.check(ctx.lib.hpe_sync(ctx.h))
    return hist.cpu().numpy().copy()


def _pipelined(ctx, frames, st, switch=None):
    """N_PIPE frames through hpe_track_pipelined; switch(f) runs before frame f."""
    import torch
    st[:26] = torch.from_numpy(oracle_np.X0)
    st[26] = 0.0
    torch.cuda.synchronize()
    ctx.pipeline_begin(frames[0])
    out = []
    for f in range(N_PIPE):
        if switch:
            switch(f)
        ctx.track_pipelined(P, 1, st.data_ptr(), frames[f + 1] if f + 1 < N_PIPE else None)
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        out.append(st.cpu().numpy().copy())
    return np.array(out)


def test_sequences_bitwise(gh, depth):
    """Captured (first pass) and replayed (second pass) chunk graphs of 8 frames, and the
    per-frame pipelined loop: every frame's 27-double state is the same bits either way."""
    import torch
    ctx = gh.ctx
    _push_params(ctx)
    _, dm = depth
    frames = [np.ascontiguousarray(dm[f + 1], dtype=np.float32) for f in range(N_SEQ)]
    d_raw = torch.from_numpy(np.stack(frames)).to("cuda:0")
    bufs = (torch.zeros(27, dtype=torch.float64, device="cuda:0"),
            torch.empty((N_SEQ, 27), dtype=torch.float64, device="cuda:0"))
    was = ctx.refine_spec
    try:
        runs = {}
        for spec in (True, False):
            ctx.refine_spec = spec
            runs[spec] = [_sequence(ctx, d_raw, bufs) for _ in range(2)]
            runs[spec].append(_pipelined(ctx, frames, bufs[0]))
    finally:
        ctx.refine_spec = was
    assert np.isfinite(runs[False][0]).all()
    for k, name in enumerate(("captured", "replayed", "pipelined")):
        a, b = runs[True][k], runs[False][k]
        bad = np.flatnonzero((_bits(a) != _bits(b)).any(axis=1))
        print(f"{name}: frames that differ {bad.tolist()}")
        assert len(bad) == 0, name
    assert np.array_equal(_bits(runs[False][0]), _bits(runs[False][1]))
    assert np.array_equal(_bits(runs[False][0][:N_PIPE]), _bits(runs[False][2]))


def test_switch_between_frames(gh, depth):
    """hpe_set_refine_spec between tracked frames (the cached graphs are rebuilt): the states
    of either setting alone."""
    import torch
    ctx = gh.ctx
    _push_params(ctx)
    _, dm = depth
    frames = [np.ascontiguousarray(dm[f + 1], dtype=np.float32) for f in range(N_PIPE)]
    st = torch.zeros(27, dtype=torch.float64, device="cuda:0")
    was = ctx.refine_spec

    def flip(f):
        ctx.refine_spec = f % 2 == 0

    try:
        ctx.refine_spec = True
        on = _pipelined(ctx, frames, st)
        ctx.refine_spec = False
        off = _pipelined(ctx, frames, st)
        mixed = _pipelined(ctx, frames, st, switch=flip)
    finally:
        ctx.refine_spec = was
    assert np.array_equal(_bits(on), _bits(off))
    assert np.array_equal(_bits(mixed), _bits(on))
