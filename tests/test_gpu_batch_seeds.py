"""Lane seeds (hpe_set_batch_seeds): every lane of the prepared, raw and live batch draws under a
seed of its own, in the workgroup form and in both wave forms.

The yardstick is never the batch: lane b is compared, bit for bit (NaNs included), with the
single-sequence call the batch call mirrors on a SEPARATE context after hpe_set_seed(seeds[b])
(tests/lane_seed_env.py).  Seeds are 1000 + b; their informant in-degrees K differ between lanes
(tests/test_batch_seeds_abi.py), so a lane that read another lane's tables would not pass.

P = 24 and P = 40, maxiter 6 (G = 5), 250-point clouds, 3 frames.
"""
import ctypes as C

import numpy as np
import pytest

import lane_seed_env as E
from lane_seed_env import NF, same, seeds_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    p = E.Pool()
    yield p
    p.close()


@pytest.fixture()
def env(pool):
    e = pool.under_test()
    yield e
    e.end_live()  # (a live batch a failed test left behind keeps what it began with)
    e.ctx.set_batch_seeds(None)
    e.ctx.set_batch_hands(None)
    e.ctx.set_batch_window("off")


def check_lanes(kind, got, own, what, n=NF):
    """The batch's result against the yardstick's own rows (n x B x 27)."""
    B = own.shape[1]
    for b in range(B):
        for f in range(n):
            row = got[f, b] if kind == "live" else got[0][b, f]
            assert same(row, own[f, b]), (what, "lane", b, "frame", f)
        if kind != "live":
            assert same(got[1][b], own[n - 1, b]), (what, "lane", b, "final state")


# ---- 1. distinct seeds in the three batch calls, default form
@pytest.mark.parametrize("P", E.P_SIZES)
@pytest.mark.parametrize("kind", ["prepared", "raw", "live"])
def test_three_seeds(pool, env, kind, P):
    seeds, streams = seeds_for(3), [0, 1, 2]
    own, _ = pool.yard(kind, P, seeds, streams, pool.start(3))
    env.ctx.set_batch_seeds(seeds)
    got = env.batch(kind, P, streams, pool.start(3))
    check_lanes(kind, got, own, (kind, P))
    assert np.isfinite(own).all()
    # the seed matters: on one stream the three seeds' yardsticks differ from one another
    one, _ = pool.yard(kind, P, seeds, [0, 0, 0], pool.start(3))
    for i in range(3):
        for j in range(i + 1, 3):
            assert not same(one[:, i], one[:, j]), (i, j)


# ---- 2. both wave forms, one and two waves per particle
@pytest.mark.parametrize("kind,wpp,P", [("raw", 2, 24), ("raw", 1, 40), ("live", 2, 40),
                                        ("live", 1, 24), ("prepared", 1, 24)])
def test_wave_form(pool, kind, wpp, P):
    # B * P <= 1024: two waves per particle on a default context; one on a context that forces it
    benv = pool.under_test(None if wpp == 2 else 1)
    assert benv.ctx.batch_wave_wpp(P, 3) == wpp
    seeds, streams = seeds_for(3), [0, 1, 2]
    own, _ = pool.yard(kind, P, seeds, streams, pool.start(3), form="wave", wpp=wpp)
    benv.ctx.set_batch_seeds(seeds)
    try:
        got = benv.batch(kind, P, streams, pool.start(3), form="wave")
    finally:
        benv.ctx.set_batch_seeds(None)
    check_lanes(kind, got, own, (kind, wpp, P))
    assert np.isfinite(own).all()
    one, _ = pool.yard(kind, P, seeds[:2], [0, 0], pool.start(2), form="wave", wpp=wpp)
    assert not same(one[:, 0], one[:, 1])


# ---- 3. indexing ends: sixteen lanes, one odd seed (the one with the larger K)
@pytest.mark.parametrize("odd", [0, 15])
def test_sixteen_lanes_one_odd_seed(pool, env, odd):
    P = 24
    seeds = [1000] * 16
    seeds[odd] = 1002
    streams = [b % 3 for b in range(16)]
    own, _ = pool.yard("raw", P, seeds, streams, pool.start(16), n=2)
    env.ctx.set_batch_seeds(seeds)
    got = env.batch("raw", P, streams, pool.start(16), n=2)
    check_lanes("raw", got, own, ("odd", odd), n=2)
    twin = 3 if odd == 0 else 12  # a lane of the odd lane's stream under the common seed
    assert streams[twin] == streams[odd] and not same(got[0][odd], got[0][twin])


# ---- 4. a permutation of the seeds permutes the results
def test_permuted_seeds(pool, env):
    P = 40
    base, perm = seeds_for(3), [2, 0, 1]
    env.ctx.set_batch_seeds(base)
    first = env.batch("raw", P, [0, 0, 0], pool.start(3))
    env.ctx.set_batch_seeds([base[k] for k in perm])
    second = env.batch("raw", P, [0, 0, 0], pool.start(3))
    for b, k in enumerate(perm):
        assert same(second[0][b], first[0][k]) and same(second[1][b], first[1][k]), (b, k)
    own, _ = pool.yard("raw", P, base, [0, 0, 0], pool.start(3))
    check_lanes("raw", first, own, "identity")


# ---- 5. the context's seed in every lane, and NULL again
@pytest.mark.parametrize("form", ["auto", "wave"])
def test_context_seed_and_null(pool, env, form):
    P, streams = 24, [0, 1, 2]
    plain = env.batch("raw", P, streams, pool.start(3), form=form)
    env.ctx.set_batch_seeds([1000] * 3)
    shared = env.batch("raw", P, streams, pool.start(3), form=form)
    assert same(shared[0], plain[0]) and same(shared[1], plain[1])
    env.ctx.set_batch_seeds(seeds_for(3))
    other = env.batch("raw", P, streams, pool.start(3), form=form)
    assert same(other[0][0], plain[0][0]) and not same(other[0][1], plain[0][1])
    env.ctx.set_batch_seeds(None)
    again = env.batch("raw", P, streams, pool.start(3), form=form)
    assert same(again[0], plain[0]) and same(again[1], plain[1])
    if form == "auto":
        own, _ = pool.yard("raw", P, [1000] * 3, streams, pool.start(3))
        check_lanes("raw", plain, own, "no seeds")


# ---- 6. new seeds between two calls of one shape; the same seeds twice capture nothing
@pytest.mark.parametrize("kind", ["raw", "live"])
def test_new_seeds_and_captures(pool, env, kind):
    P, streams = 40, [0, 1, 2]
    a, b = seeds_for(3), [1003, 1001, 1004]
    own_a, _ = pool.yard(kind, P, a, streams, pool.start(3))
    own_b, _ = pool.yard(kind, P, b, streams, pool.start(3))
    env.ctx.set_batch_seeds(a)
    first = env.batch(kind, P, streams, pool.start(3), tag="cap")
    c = env.ctx.graph_captures()
    twice = env.batch(kind, P, streams, pool.start(3), tag="cap")
    assert env.ctx.graph_captures() == c
    env.ctx.set_batch_seeds(a)  # set again, unchanged
    thrice = env.batch(kind, P, streams, pool.start(3), tag="cap")
    assert env.ctx.graph_captures() == c
    env.ctx.set_batch_seeds(b)
    second = env.batch(kind, P, streams, pool.start(3), tag="cap")
    c2 = env.ctx.graph_captures()
    again = env.batch(kind, P, streams, pool.start(3), tag="cap")
    assert env.ctx.graph_captures() == c2
    check_lanes(kind, first, own_a, "first")
    check_lanes(kind, twice, own_a, "twice")
    check_lanes(kind, thrice, own_a, "thrice")
    check_lanes(kind, second, own_b, "new seeds")
    check_lanes(kind, again, own_b, "new seeds again")
    assert same(own_a[:, 1], own_b[:, 1]) and not same(own_a[:, 0], own_b[:, 0])


# ---- 7. seeds together with lane hands and a FIXED window
def test_seeds_with_hands_and_a_fixed_window(pool, env):
    P, names, seeds, streams = 24, ["A", "S"], [1001, 1002], [0, 1]
    wins = [pool.single(seeds[b], name=names[b]).ctx.window_from_pose(env.x0, E.FOCAL, 2.0, 4.0)
            for b in range(2)]
    assert wins[0] != wins[1] and not any(env.hpe.window.is_whole(w) for w in wins)
    x, own = pool.start(2), []
    for f in range(NF):
        x = np.stack([pool.step("raw", P, seeds[b], streams[b], f, x[b], name=names[b],
                                window=wins[b]) for b in range(2)])
        own.append(x)
    own = np.array(own)
    env.ctx.set_batch_hands([pool.single(seeds[b], name=names[b]).hand for b in range(2)])
    env.ctx.set_batch_window("fixed", wins)
    env.ctx.set_batch_seeds(seeds)
    got = env.batch("raw", P, streams, pool.start(2))
    check_lanes("raw", got, own, "hands + window")
    assert np.isfinite(own).all()
    # the window and the hand matter to the yardstick
    bare = pool.step("raw", P, seeds[1], streams[1], 0, pool.start(1)[0])
    assert not same(bare, own[0, 1])


# ---- 8. refusals change nothing
def test_refusals_change_nothing(pool, env):
    _lib, lib, h = env.hpe._lib, env.lib, env.ctx.h
    M, P = _lib.BATCH_MAX, 24
    seeds, streams = seeds_for(2), [0, 1]
    own, _ = pool.yard("raw", P, seeds, streams, pool.start(2))
    live, _ = pool.yard("live", P, seeds, streams, pool.start(2))

    def err():
        return lib.hpe_last_error(h)

    def still():
        check_lanes("raw", env.batch("raw", P, streams, pool.start(2)), own, "still")

    env.ctx.set_batch_seeds(seeds)
    still()
    arr = (C.c_uint64 * (M + 1))(*range(2000, 2000 + M + 1))
    for B in (0, -1, M + 1):
        assert lib.hpe_set_batch_seeds(h, B, arr) == _lib.HPE_E_ARG and b"lanes" in err()
    assert lib.hpe_set_batch_seeds(None, 2, arr) == _lib.HPE_E_ARG
    still()
    # a batch call or begin with another lane count than the seeds'
    t = env.torch
    st = t.zeros((3, 27), dtype=t.float64, device="cuda:0")
    st[:, :26] = t.from_numpy(env.x0)
    t.cuda.synchronize()
    before = st.cpu().numpy()
    raws3 = (C.c_void_p * 3)(*[pool.raw(0).data_ptr()] * 3)
    assert lib.hpe_track_raw_batch_dev(h, P, 1, 3, C.c_void_p(st.data_ptr()), raws3, NF, 1, 1, E.FOCAL,
                                       2, None) == _lib.HPE_E_ARG and b"seeds were set for 2" in err()
    s0 = env.slot0(0)
    slots3 = (C.c_int32 * 3)(s0, s0, s0)
    assert lib.hpe_track_batch_dev(h, P, 1, 3, C.c_void_p(st.data_ptr()), slots3, NF, 2,
                                   None) == _lib.HPE_E_ARG and b"seeds were set for 2" in err()
    f0 = pool.frames(0)[0]
    fr3 = (C.c_void_p * 3)(*[f0.ctypes.data] * 3)
    assert lib.hpe_batch_pipeline_begin(h, 3, fr3, 1, 1, E.FOCAL) == _lib.HPE_E_ARG
    assert b"seeds were set for 2" in err()
    env.sync()
    assert same(st.cpu().numpy(), before)
    still()
    # a live batch in progress keeps the seeds it began with: every set is refused, NULL included
    fr = [pool.frames(s) for s in streams]
    st2 = t.zeros((2, 27), dtype=t.float64, device="cuda:0")
    st2[:, :26] = t.from_numpy(env.x0)
    t.cuda.synchronize()
    env.ctx.batch_pipeline_begin([x[0] for x in fr])
    assert lib.hpe_set_batch_seeds(h, 2, arr) == _lib.HPE_E_STATE and b"live batch" in err()
    assert lib.hpe_set_batch_seeds(h, 0, None) == _lib.HPE_E_STATE and b"live batch" in err()
    for f in range(NF):
        env.ctx.track_batch_pipelined(P, 1, st2.data_ptr(), [x[f + 1] for x in fr] if f + 1 < NF else None)
        env.sync()
        got = st2.cpu().numpy()
        for b in range(2):
            assert same(got[b], live[f, b]), (f, b)
    still()
    assert lib.hpe_set_batch_seeds(h, 0, None) == 0  # the batch has ended
