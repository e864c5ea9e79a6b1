"""The self-collision term's 144 sphere pairs (costfunc.cpp:130-197) on fat-sphere hands.

At the reference radii a pose activates about one of the 144 pairs, so a wrong pair map
passes unnoticed.  hand_data.collision_cases() scales the radii by 1.5 to 4: over the list
every pair is active in one case and inactive in another (asserted here), and on every case
the two oracles and a per-pair restatement written here agree on the collision sum.

pair_values / collision_sum below are the reference of tests/test_gpu_collision.py too.
"""
from pathlib import Path

import numpy as np
import pytest

import hand_data
import oracle_np

NPAIR = 144


def pair_rows():
    """(a, b) of the 144 pairs: digit pair p = t // 36 (thumb-index .. ring-little), whose
    rows 2 + 10 p + 0..5 (the reference's smat1, each row repeated 6 times: k // 6) meet rows
    2 + 10 (p + 1) + 0..5 (smat2, the 6 rows tiled 6 times: k % 6)."""
    p, k = np.divmod(np.arange(NPAIR), 36)
    return 2 + 10 * p + k // 6, 2 + 10 * (p + 1) + k % 6


def pair_values(S, radii):
    """v[t] = (r_b + r_a) - |S_b - S_a| of the 144 pairs (costfunc.cpp:186-189): pair t is
    active, and adds v[t]^2, where v[t] > 0."""
    a, b = pair_rows()
    S, r = np.asarray(S, dtype=np.float64), np.asarray(radii, dtype=np.float64)
    d = S[b] - S[a]
    return (r[b] + r[a]) - np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def collision_sum(v):
    """costfunc.cpp:190-192: per digit pair, the squares of the positive values summed in
    Armadillo's order (two interleaved accumulators), the four sums added in turn."""
    pen = 0.0
    for p in range(4):
        blk = v[36 * p:36 * p + 36]
        sq = [float(x) * float(x) for x in blk[blk > 0]]
        a1 = a2 = 0.0
        for i in range(0, len(sq) - 1, 2):
            a1 += sq[i]
            a2 += sq[i + 1]
        if len(sq) % 2:
            a1 += sq[-1]
        pen += a1 + a2
    return pen


@pytest.fixture(scope="module")
def cases(oracle, ora_hand):
    """[(radius scale, theta, S)]: FK does not read the radii, so the reference hand's."""
    return [(k, th, oracle.build(ora_hand, th)) for k, th in hand_data.collision_cases()]


def test_pair_rows_are_the_reference_repmat():
    """The index formula against the reference's own construction: repmat(smat1.t(), 6, 1)
    reshaped to 3 x 36 and transposed repeats each of the six rows six times; repmat(smat2,
    6, 1) tiles the six rows six times."""
    a, b = pair_rows()
    S = np.arange(48 * 3, dtype=np.float64).reshape(48, 3)  # every coordinate names its row
    base = (2, 12, 22, 32, 42)
    for p in range(4):
        m1, m2 = S[base[p]:base[p] + 6], S[base[p + 1]:base[p + 1] + 6]
        smat1 = np.tile(m1.T, (6, 1)).reshape((3, 36), order="F").T  # Armadillo: column-major
        smat2 = np.tile(m2, (6, 1))
        assert np.array_equal(smat1, S[a[36 * p:36 * p + 36]])
        assert np.array_equal(smat2, S[b[36 * p:36 * p + 36]])
    assert len(set(zip(a.tolist(), b.tolist()))) == NPAIR


def test_every_pair_in_both_states(cases):
    """The coverage condition of the case list: each of the 144 pairs is active (v > 0) in at
    least one case and inactive in at least one."""
    rad = hand_data.geometry_cm()[1]
    act = np.array([pair_values(S, rad * k) > 0 for k, _, S in cases])
    scales = np.array([k for k, _, _ in cases])
    for k in sorted(set(scales.tolist())):
        m = act[scales == k]
        print("scale %g: %d cases, %d pairs active, %d in both states, %.1f active per pose"
              % (k, len(m), m.any(0).sum(), (m.any(0) & ~m.all(0)).sum(), m.sum(1).mean()))
    print("all: %d cases, %d active, %d in both states"
          % (len(act), act.any(0).sum(), (act.any(0) & ~act.all(0)).sum()))
    assert set(scales.tolist()) == {1.5, 2.0, 3.0, 4.0}
    assert len(cases) <= 40
    never, always = np.flatnonzero(~act.any(0)), np.flatnonzero(act.all(0))
    assert len(never) == 0 and len(always) == 0, (never, always)


def test_collision_share_of_the_cost(oracle):
    """On the frames of tests/test_gpu_collision.py (each scale's hand rendered at the centre
    pose, 250 points) the collision term is at least a tenth of cal_cost2 in at least half the
    cases: the totals compared there cannot hide the term."""
    geo, rad = hand_data.geometry_cm()
    cases = hand_data.collision_cases()
    shares = []
    for k in sorted({k for k, _ in cases}):
        d = oracle_np.render_depth_mm(oracle_np.Hand(geo, rad * k), hand_data.collision_centre())
        obs = oracle.preprocess(d, downsample=True)
        h = oracle.hand(geo, rad * k)
        for kk, th in cases:
            if kk == k:
                c, t, _ = oracle.terms(h, obs, th)
                shares.append(t[2] / c)
                print("scale %g: collision %.4g of %.4g (%.3f)" % (k, t[2], c, t[2] / c))
    assert len(shares) == len(cases)
    assert 2 * sum(s >= 0.1 for s in shares) >= len(shares), shares


def test_three_restatements_agree(oracle, cases):
    """The C oracle, the numpy oracle and the per-pair restatement on every case, at the
    tolerance test_golden.py uses between restatements."""
    geo, rad = hand_data.geometry_cm()
    f = np.load(Path(__file__).resolve().parent / "golden" / "frame.npz", allow_pickle=False)
    obs = oracle.preprocess(f["depth_mm"], downsample=True)
    obs_np = oracle_np.Obs(obs.depth, obs.dt, obs.cloud, obs.scale, K=obs.K.reshape(3, 3))
    hands = {}
    for k, th, S in cases:
        if k not in hands:
            hands[k] = (oracle.hand(geo, rad * k), oracle_np.Hand(geo, rad * k))
        hc, hn = hands[k]
        c_c = oracle.terms(hc, obs, th)[1][2]
        c_np = oracle_np.cal_cost2(hn, obs_np, th)[2][2]
        c_pair = collision_sum(pair_values(S, rad * k))
        assert c_pair > 0
        assert abs(c_c - c_pair) <= 1e-12 * c_pair, (k, c_c, c_pair)
        assert abs(c_np - c_pair) <= 1e-12 * c_pair, (k, c_np, c_pair)
        assert abs(c_c - c_np) <= 1e-12 * c_pair, (k, c_c, c_np)
