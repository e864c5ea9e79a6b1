"""Lane groups (hpe_set_batch_groups, hpe_batch_group_pick, hpe_batch_group_rows): runs of
consecutive lanes exchange their best pose after every tracked frame.

The pick rule is checked on crafted rows against hpe.group.pick.  Tracked groups are checked
against a yardstick that uses no code of lane seeds or groups (tests/lane_seed_env.py): one
context per seed after hpe_set_seed, frame f of lane b the single-sequence call on that one frame
from the row x_{f-1}, and x_f hpe.dist.pick_best over the group's own rows.  Own rows
(hpe_batch_group_rows), d_states and d_hist must equal it bit for bit, NaNs included.

P = 24 and P = 40, maxiter 6 (G = 5), 250-point clouds, 3 frames; lane b's seed is 1000 + b.
"""
import ctypes as C

import numpy as np
import pytest

import lane_seed_env as E
from lane_seed_env import NF, same, seeds_for

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
MXY, MZ = 2.0, 4.0


@pytest.fixture(scope="module")
def pool():
    p = E.Pool()
    yield p
    p.close()


@pytest.fixture()
def env(pool):
    e = pool.under_test()
    yield e
    e.end_live()  # (a live batch a failed test left behind keeps its settings)
    e.ctx.set_batch_groups(None)
    e.ctx.set_batch_seeds(None)
    e.ctx.set_batch_window("off")
    e.ctx.set_batch_report(0)
    e.ctx.set_batch_pacing("lockstep")


def grouped(env, seeds, sizes):
    env.ctx.set_batch_seeds(seeds)
    env.ctx.set_batch_groups(sizes)


def check_resident(env, got, own, picked, n, what):
    hist, st = got
    B = st.shape[0]
    for b in range(B):
        for f in range(n):
            assert same(hist[b, f], picked[f, b]), (what, "hist", b, f)
    assert same(st, picked[n - 1]), (what, "states")
    assert same(env.ctx.batch_group_rows(B), own[n - 1]), (what, "own rows")


# ---- 1. the pick rule on crafted rows
def crafted(costs):
    r = np.zeros((len(costs), 27))
    r[:, :26] = np.arange(1, len(costs) + 1)[:, None] + np.arange(26)[None, :] / 32.0
    r[:, 26] = costs
    return r


COSTS16 = [5.0, 4.0, NAN, 9.0, 2.0, 2.0, 7.0, INF, -3.0, 8.0, NAN, 6.0, -3.0, 1.0, 0.5, 3.0]


@pytest.mark.parametrize("sizes,costs", [
    ([1], [NAN]), ([1], [2.5]),
    ([16], COSTS16), ([3, 1, 12], COSTS16),
    ([4], [3.0, 1.0, 1.0, 2.0]),                # a tie between different poses: the lowest lane
    ([3], [NAN, INF, NAN]),                     # a NaN cost loses to +inf
    ([3, 2], [NAN, NAN, NAN, NAN, 1.0]),        # an all-NaN group takes its lowest lane
    ([4], [0.0, -1e300, -INF, -INF]),           # -inf wins
    ([2, 2], [0.0, -0.0, 7.0, 7.0]),
])
def test_group_pick_on_crafted_rows(env, sizes, costs):
    from hpe import group
    B, t = len(costs), env.torch
    rows = crafted(costs)
    if sizes == [3, 2]:
        rows[0, 5] = NAN  # a NaN pose travels with its row
    tail = crafted([11.0, NAN, -INF])  # rows outside the call's groups
    buf = t.from_numpy(np.vstack([rows, tail])).to("cuda:0")
    env.ctx.set_batch_groups(sizes)
    env.ctx.batch_group_pick(buf.data_ptr(), B)
    env.sync()
    got = buf.cpu().numpy()
    assert same(got[:B], group.pick(rows, sizes))
    assert same(got[B:], tail)
    # picking again changes nothing
    env.ctx.batch_group_pick(buf.data_ptr(), B)
    env.sync()
    assert same(buf.cpu().numpy(), got)


# ---- 2. tracked groups over two streams in the three batch calls
CASES = [(24, [2, 2], [0, 0, 1, 1]), (40, [3, 1], [0, 0, 0, 1])]


@pytest.mark.parametrize("P,sizes,streams", CASES)
@pytest.mark.parametrize("kind", ["prepared", "raw"])
def test_tracked_groups_resident(pool, env, kind, P, sizes, streams):
    seeds = seeds_for(4)
    own, picked = pool.yard(kind, P, seeds, streams, pool.start(4), sizes)
    grouped(env, seeds, sizes)
    for n in (1, 2, 3):  # the own rows are the last frame's
        got = env.batch(kind, P, streams, pool.start(4), n=n)
        check_resident(env, got, own, picked, n, (kind, P, n))
    assert np.isfinite(own).all()
    # the pick matters: some lane's own row is not the row it carries on
    assert not same(own, picked)
    free, _ = pool.yard(kind, P, seeds, streams, pool.start(4))
    assert not same(free[NF - 1], own[NF - 1])


@pytest.mark.parametrize("P,sizes,streams", CASES)
def test_tracked_groups_live(pool, env, P, sizes, streams):
    seeds = seeds_for(4)
    own, picked = pool.yard("live", P, seeds, streams, pool.start(4), sizes)
    grouped(env, seeds, sizes)
    rows = []
    got = env.batch("live", P, streams, pool.start(4), after=lambda f: rows.append(env.ctx.batch_group_rows(4)))
    for f in range(NF):
        assert same(got[f], picked[f]), ("states", f)
        assert same(rows[f], own[f]), ("own rows", f)
    assert not same(own, picked)


# ---- 3. one group of sixteen
def test_one_group_of_sixteen(pool, env):
    P, seeds, streams = 24, seeds_for(16), [0] * 16
    own, picked = pool.yard("raw", P, seeds, streams, pool.start(16), [16], n=2)
    grouped(env, seeds, [16])
    got = env.batch("raw", P, streams, pool.start(16), n=2)
    check_resident(env, got, own, picked, 2, "sixteen")
    assert len({own[0, b].tobytes() for b in range(16)}) == 16


# ---- 4. the wave form
@pytest.mark.parametrize("kind,wpp", [("raw", 2), ("live", 1)])
def test_wave_form(pool, kind, wpp):
    P, sizes, streams, seeds = 40, [2, 2], [0, 0, 1, 1], seeds_for(4)
    benv = pool.under_test(None if wpp == 2 else 1)
    assert benv.ctx.batch_wave_wpp(P, 4) == wpp
    own, picked = pool.yard(kind, P, seeds, streams, pool.start(4), sizes, form="wave", wpp=wpp)
    grouped(benv, seeds, sizes)
    try:
        rows = []
        got = benv.batch(kind, P, streams, pool.start(4), form="wave",
                         after=lambda f: rows.append(benv.ctx.batch_group_rows(4)))
        if kind == "live":
            for f in range(NF):
                assert same(got[f], picked[f]) and same(rows[f], own[f]), f
        else:
            check_resident(benv, got, own, picked, NF, ("wave", wpp))
    finally:
        benv.ctx.set_batch_groups(None)
        benv.ctx.set_batch_seeds(None)
    assert not same(own, picked)


# ---- 5. equal seeds: every own row of a group is the same, and the pick changes no bits
def test_groups_with_equal_seeds(pool, env):
    P, streams = 24, [0, 0, 1, 1]
    plain = env.batch("raw", P, streams, pool.start(4))
    env.ctx.set_batch_groups([2, 2])
    got = env.batch("raw", P, streams, pool.start(4))
    assert same(got[0], plain[0]) and same(got[1], plain[1])
    assert same(env.ctx.batch_group_rows(4), plain[1])
    assert same(plain[0][0], plain[0][1]) and not same(plain[0][0], plain[0][2])


# ---- 6. a lane started from a NaN pose never wins
def test_a_nan_lane_never_wins(pool, env):
    P, sizes, streams, seeds = 24, [2, 1], [0, 0, 0], seeds_for(3)
    starts = pool.start(3)
    starts[0, :26] = NAN
    own, picked = pool.yard("raw", P, seeds, streams, starts, sizes)
    # (the lane's own result of frame 0 is whatever the single call makes of a NaN pose)
    assert np.isfinite(own[:, 1:]).all() and not same(own[0, 0], own[0, 1])
    grouped(env, seeds, sizes)
    got = env.batch("raw", P, streams, starts)
    check_resident(env, got, own, picked, NF, "nan lane")
    assert np.isfinite(got[0]).all() and same(got[0][0, 0], own[0, 1])


# ---- 7. groups of one lane equal no groups
def test_groups_of_one_equal_no_groups(pool, env):
    P, streams, seeds = 40, [0, 1, 2], seeds_for(3)
    env.ctx.set_batch_seeds(seeds)
    plain = env.batch("raw", P, streams, pool.start(3))
    env.ctx.set_batch_groups([1, 1, 1])
    got = env.batch("raw", P, streams, pool.start(3))
    assert same(got[0], plain[0]) and same(got[1], plain[1])
    assert same(env.ctx.batch_group_rows(3), plain[1])
    env.ctx.set_batch_groups(None)
    live_plain = env.batch("live", P, streams, pool.start(3))
    env.ctx.set_batch_groups([1, 1, 1])
    live = env.batch("live", P, streams, pool.start(3))
    assert same(live, live_plain)


# ---- 8. free pacing: a group advances as one
def test_free_pacing(pool, env):
    P, sizes, streams, seeds = 24, [2, 2], [0, 0, 1, 1], seeds_for(4)
    fr = [pool.frames(s) for s in streams]
    own, picked = pool.yard("live", P, seeds, streams, pool.start(4), sizes, n=2)
    grouped(env, seeds, sizes)
    env.ctx.set_batch_pacing("free")
    st, _ = env.bufs_for(4, NF, "free")
    st.copy_(env.torch.from_numpy(pool.start(4)))
    env.torch.cuda.synchronize()
    refused = f"hpe error {env.hpe._lib.HPE_E_ARG}: .*a group advances as one"
    # a split group is refused, in the begin and in a track call, and nothing changes
    with pytest.raises(env.hpe.HpeError, match=refused):
        env.ctx.batch_pipeline_begin([fr[0][0], None, fr[2][0], fr[3][0]])
    env.ctx.batch_pipeline_begin([x[0] for x in fr])
    with pytest.raises(env.hpe.HpeError, match=refused):
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [fr[0][1], fr[1][1], None, fr[3][1]])
    assert env.ctx.batch_pending() == 0b1111
    # call 1: both groups track frame 0; only group 0 is given a next frame
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [fr[0][1], fr[1][1], None, None])
    env.sync()
    s1, r1 = st.cpu().numpy().copy(), env.ctx.batch_group_rows(4)
    assert same(s1, picked[0]) and same(r1, own[0])
    assert env.ctx.batch_pending() == 0b0011
    # call 2: group 0 tracks frame 1, group 1 idles: its rows of both tables stay bit for bit
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [None, None, fr[2][1], fr[3][1]])
    env.sync()
    s2, r2 = st.cpu().numpy().copy(), env.ctx.batch_group_rows(4)
    assert same(s2[:2], picked[1][:2]) and same(r2[:2], own[1][:2])
    assert same(s2[2:], s1[2:]) and same(r2[2:], r1[2:])
    # call 3: group 1 tracks its frame 1 from the rows it kept; group 0 idles
    env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), None)
    env.sync()
    s3, r3 = st.cpu().numpy().copy(), env.ctx.batch_group_rows(4)
    assert same(s3[2:], picked[1][2:]) and same(r3[2:], own[1][2:])
    assert same(s3[:2], s2[:2]) and same(r3[:2], r2[:2])


# ---- 9. FOLLOW windows follow the picked pose
def test_follow_windows_from_the_picked_row(pool, env):
    from hpe import dist, window
    import torch
    P, seeds, streams = 40, seeds_for(2), [0, 0]
    hand = env.hand
    radii = np.asarray(hand.spheres_radii, dtype=np.float64)

    def rule(theta):
        return window.from_spheres(hand.build_hand_model(np.asarray(theta)[:26]), radii, E.FOCAL, MXY, MZ)

    def pick(rows):
        return np.stack([dist.pick_best(torch.from_numpy(rows)).numpy()] * 2)

    w0 = rule(env.x0)
    x, wins, own, picked = pool.start(2), [w0, w0], [], []
    for f in range(NF):  # frame f >= 2 is read through the window of the rows after frame f - 2
        if f >= 2:
            assert rule(picked[f - 2][0]) == rule(picked[f - 2][1])
            wins.append(rule(picked[f - 2][0]))
        rows = np.stack([pool.step("raw", P, seeds[b], 0, f, x[b], window=wins[f]) for b in range(2)])
        x = pick(rows)
        own.append(rows)
        picked.append(x)
    own, picked = np.array(own), np.array(picked)
    grouped(env, seeds, [2])
    env.ctx.set_batch_window("follow", [w0, w0], MXY, MZ)
    got = env.batch("raw", P, streams, pool.start(2))
    check_resident(env, got, own, picked, NF, "follow")
    tab = env.ctx.batch_windows_readback((NF - 1) & 1, 2)
    assert tab[0] == tab[1] == wins[NF - 1]
    assert wins[2] != w0 and not same(own[0, 0], own[0, 1])


# ---- 10. reports carry the picked row
def test_reports_carry_the_picked_row(pool, env):
    P, sizes, streams, seeds = 24, [2, 2], [0, 0, 1, 1], seeds_for(4)
    _, picked = pool.yard("live", P, seeds, streams, pool.start(4), sizes)
    grouped(env, seeds, sizes)
    env.ctx.set_batch_report(4)
    seen = []
    got = env.batch("live", P, streams, pool.start(4),
                    after=lambda f: seen.append([env.ctx.batch_report(b).state for b in range(4)]))
    for f in range(NF):
        assert same(got[f], picked[f]), f
        assert same(np.array(seen[f]), picked[f]), ("reports", f)


# ---- 11. the optimiser over a group, the pick, then tracked frames
def test_optimise_pick_then_track(pool, env):
    import torch
    from hpe import dist
    P, sizes, streams, seeds = 24, [2, 2], [0, 0, 1, 1], seeds_for(4)
    fr = [pool.frames(s) for s in streams]
    starts = pool.start(4)
    starts[1, :26] += 0.5   # the optimiser keeps the context's seed: the lanes differ by their starts
    starts[3, 3:6] += 1.0
    grouped(env, seeds, sizes)
    st, _ = env.bufs_for(4, NF, "opt")
    st.copy_(env.torch.from_numpy(starts))
    env.torch.cuda.synchronize()
    env.ctx.batch_pipeline_begin([x[0] for x in fr])
    env.ctx.batch_pipeline_optimise(P, st.data_ptr())
    env.sync()
    opt = st.cpu().numpy().copy()
    assert not same(opt[0], opt[1]) and not same(opt[2], opt[3])
    want = opt.copy()
    for a in (0, 2):
        want[a:a + 2] = dist.pick_best(torch.from_numpy(opt[a:a + 2])).numpy()
    env.ctx.batch_group_pick(st.data_ptr(), 4)
    env.sync()
    assert same(st.cpu().numpy(), want)
    own, picked = pool.yard("live", P, seeds, streams, want, sizes)
    for f in range(NF):
        env.ctx.track_batch_pipelined(P, 1, st.data_ptr(), [x[f + 1] for x in fr] if f + 1 < NF else None)
        env.sync()
        assert same(st.cpu().numpy(), picked[f]), f
        assert same(env.ctx.batch_group_rows(4), own[f]), f


# ---- 12. the second batch of one shape captures nothing
@pytest.mark.parametrize("kind", ["prepared", "raw", "live"])
def test_graph_captures(pool, env, kind):
    P, sizes, streams, seeds = 24, [2, 2], [0, 0, 1, 1], seeds_for(4)
    grouped(env, seeds, sizes)
    first = env.batch(kind, P, streams, pool.start(4), tag="cap")
    c = env.ctx.graph_captures()
    second = env.batch(kind, P, streams, pool.start(4), tag="cap")
    assert env.ctx.graph_captures() == c
    env.ctx.set_batch_groups([3, 1])  # other groups of one shape: the table, not the graphs
    third = env.batch(kind, P, streams, pool.start(4), tag="cap")
    assert env.ctx.graph_captures() == c
    if kind == "live":
        assert same(first, second) and not same(first, third)
    else:
        assert same(first[0], second[0]) and same(first[1], second[1]) and not same(first[0], third[0])


# ---- 13. refusals change nothing
def test_refusals_change_nothing(pool, env):
    _lib, lib, h = env.hpe._lib, env.lib, env.ctx.h
    M, P = _lib.BATCH_MAX, 24
    sizes, streams, seeds = [2, 1], [0, 0, 1], seeds_for(3)
    own, picked = pool.yard("raw", P, seeds, streams, pool.start(3), sizes)

    def err():
        return lib.hpe_last_error(h)

    def z(*v):
        return (C.c_int32 * len(v))(*v)

    def still():
        check_resident(env, env.batch("raw", P, streams, pool.start(3)), own, picked, NF, "still")

    rows = np.full((3, 27), 5.0)
    rp = rows.ctypes.data_as(_lib.dp)
    t = env.torch
    st = t.zeros((4, 27), dtype=t.float64, device="cuda:0")
    st[:, :26] = t.from_numpy(env.x0)
    t.cuda.synchronize()
    before = st.cpu().numpy()
    sp = C.c_void_p(st.data_ptr())
    # nothing set yet
    assert lib.hpe_batch_group_pick(h, 3, sp) == _lib.HPE_E_STATE and b"no lane groups" in err()
    assert lib.hpe_batch_group_rows(h, 3, rp) == _lib.HPE_E_STATE
    grouped(env, seeds, sizes)
    assert lib.hpe_batch_group_rows(h, 3, rp) == _lib.HPE_E_STATE and b"no grouped frame" in err()
    assert (rows == 5.0).all()
    still()
    for B, n, s in ((0, 1, z(1)), (M + 1, 1, z(M + 1)), (3, 2, z(2, 2)), (3, 2, z(3, 0)),
                    (3, 2, z(4, -1)), (3, 2, z(1, 1)), (3, -1, z(3)), (3, 4, z(1, 1, 1, 1))):
        assert lib.hpe_set_batch_groups(h, B, n, s) == _lib.HPE_E_ARG, (B, n, list(s))
    assert lib.hpe_set_batch_groups(None, 3, 2, z(2, 1)) == _lib.HPE_E_ARG
    still()
    for B in (0, M + 1):
        assert lib.hpe_batch_group_pick(h, B, sp) == _lib.HPE_E_ARG
        assert lib.hpe_batch_group_rows(h, B, rp) == _lib.HPE_E_ARG
    assert lib.hpe_batch_group_pick(h, 3, None) == _lib.HPE_E_ARG and b"null" in err()
    assert lib.hpe_batch_group_rows(h, 3, None) == _lib.HPE_E_ARG and b"null" in err()
    assert lib.hpe_batch_group_pick(h, 4, sp) == _lib.HPE_E_ARG and b"set for 3" in err()
    assert lib.hpe_batch_group_rows(h, 2, rp) == _lib.HPE_E_ARG and b"set for 3" in err()
    # a batch call or begin with another lane count than the groups'
    env.ctx.set_batch_seeds(None)
    raws4 = (C.c_void_p * 4)(*[pool.raw(0).data_ptr()] * 4)
    assert lib.hpe_track_raw_batch_dev(h, P, 1, 4, sp, raws4, NF, 1, 1, E.FOCAL, 2,
                                       None) == _lib.HPE_E_ARG and b"groups were set for 3" in err()
    s0 = env.slot0(0)
    assert lib.hpe_track_batch_dev(h, P, 1, 4, sp, z(s0, s0, s0, s0), NF, 2,
                                   None) == _lib.HPE_E_ARG and b"groups were set for 3" in err()
    f0 = pool.frames(0)[0]
    fr4 = (C.c_void_p * 4)(*[f0.ctypes.data] * 4)
    assert lib.hpe_batch_pipeline_begin(h, 4, fr4, 1, 1, E.FOCAL) == _lib.HPE_E_ARG
    assert b"groups were set for 3" in err()
    env.sync()
    assert same(st.cpu().numpy(), before) and (rows == 5.0).all()
    env.ctx.set_batch_seeds(seeds)
    still()
    # a live batch in progress keeps the groups it began with: every set is refused, off included
    fr = [pool.frames(s) for s in streams]
    live_own, live_picked = pool.yard("live", P, seeds, streams, pool.start(3), sizes)
    st3 = t.from_numpy(pool.start(3)).to("cuda:0")
    env.ctx.batch_pipeline_begin([x[0] for x in fr])
    assert lib.hpe_set_batch_groups(h, 3, 3, z(1, 1, 1)) == _lib.HPE_E_STATE and b"live batch" in err()
    assert lib.hpe_set_batch_groups(h, 0, 0, None) == _lib.HPE_E_STATE and b"live batch" in err()
    for f in range(NF):
        env.ctx.track_batch_pipelined(P, 1, st3.data_ptr(), [x[f + 1] for x in fr] if f + 1 < NF else None)
        env.sync()
        assert same(st3.cpu().numpy(), live_picked[f]), f
        assert same(env.ctx.batch_group_rows(3), live_own[f]), f
    assert lib.hpe_set_batch_groups(h, 0, 0, None) == 0  # the batch has ended
    assert lib.hpe_batch_group_pick(h, 3, sp) == _lib.HPE_E_STATE
