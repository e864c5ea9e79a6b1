"""The hand family (hand_data.hand_family) on the CPU: the two oracle restatements against each
other on every hand, and hpe::build_dev_hand's constants against the C oracle's.

* oracle.build (C) against oracle_np.Hand.build_hand_model (numpy), spheres and joints, at
  hand_data.family_poses(): 1e-12 cm (the two sum the same products in the same order and differ
  by the libm calls numpy's and C's sin/cos share, measured 3.2e-15; the GPU tolerance is 1e-9).
  Every hand but `ref` moves an X0 sphere by more than 0.1 cm: an entry that changes nothing
  tests nothing.
* every DevHand constant of every family hand (tests/cpp/dev_hand_dump.cpp, the fixture of
  tests/test_batch_hands_abi.py) against the F and T10 matrices ora_hand_init fills, the thumb's
  pCMC twist, geo, radii and a direct restatement of the sphere-placement rule.  Both sides run
  the same libm on the same host: the test prints whether they agree bit for bit and asserts
  4 ulp of the larger magnitude; the integer tables are equal.
"""
import math

import numpy as np
import pytest

import hand_data
import oracle_np

FAMILY = hand_data.FAMILY
FK_TOL = 1e-12


@pytest.fixture(scope="module")
def family():
    return hand_data.hand_family()


def test_family_names_and_shapes(family):
    assert tuple(family) == FAMILY
    geo, rad = hand_data.geometry_cm()
    for name, (g, r, c, s) in family.items():
        assert g.shape == (20,) and r.shape == (48,) and c.shape == (5,) and s.shape == (5,), name
        assert np.isfinite(np.concatenate([g, r, c, s])).all() and (g > 0).all() and (r > 0).all()
    g, r, c, s = family["ref"]
    assert np.array_equal(g, geo) and np.array_equal(r, rad)
    assert tuple(c) == oracle_np.CMC and tuple(s) == oracle_np.SPACING
    # what the reference hand hides
    assert family["ref"][3][2] == 0 and family["uneven"][3][2] != 0
    assert np.array_equal(family["mirror"][3], -s) and not family["zero_sp"][3].any()
    assert tuple(family["right_angle"][2]) == (150.0, 90.0, 90.0, 90.0, 45.0)


def test_family_parameters_reach_the_binding(family):
    """family_gpu_hand(params_only=True) hands hpe_set_batch_hands the entry's own doubles."""
    import hpe
    for name, (g, r, c, s) in family.items():
        p = hand_data.family_gpu_hand(family[name], params_only=True)
        assert isinstance(p, hpe._lib.HandParams)
        assert np.array_equal(p.geo_cm[:], g) and np.array_equal(p.radii_cm[:], r), name
        assert np.array_equal(p.cmc_deg[:], c) and np.array_equal(p.spacing_cm[:], s), name
        assert tuple(p.tb_spheres[:]) == (2, 2, 2, 2) and tuple(p.fg_spheres[:]) == (4, 2, 2, 2)
    assert bytes(hand_data.family_gpu_hand(family["ref"], params_only=True)) == \
        bytes(hpe.scaled_hand_params(1.0))


@pytest.mark.parametrize("name", FAMILY)
def test_oracle_c_against_oracle_np(oracle, family, name):
    ora, nph = hand_data.family_oracle_hands(oracle, family[name])
    poses = hand_data.family_poses()
    assert poses.shape == (17, 26)
    worst = 0.0
    for th in poses:
        Sc, Jc = oracle.build(ora, th, joints=True)
        Sn, Jn = nph.build_hand_model(th, return_joints=True)
        assert np.isfinite(Sc).all() and np.isfinite(Jc).all()
        worst = max(worst, np.abs(Sc - Sn).max(), np.abs(Jc - Jn).max())
    ref, _ = hand_data.family_oracle_hands(oracle, family["ref"])
    moved = np.abs(oracle.build(ora, oracle_np.X0) - oracle.build(ref, oracle_np.X0)).max()
    print(f"hand {name}: C oracle vs numpy oracle {worst:.3g} cm over {len(poses)} poses; "
          f"X0 spheres moved {moved:.3g} cm from the reference hand's")
    assert worst <= FK_TOL
    if name != "ref":
        assert moved > 0.1


# ---- build_dev_hand against the oracle's constants
@pytest.fixture(scope="module")
def dev_family(tmp_path_factory, family):
    ps = [hand_data.family_gpu_hand(family[n], params_only=True) for n in FAMILY]
    hands, stdout = hand_data.dev_hand_dump(tmp_path_factory.mktemp("dhf"), ps)
    assert f"{len(FAMILY)} hands of 2016 bytes" in stdout
    return dict(zip(FAMILY, hands))


def _placement():
    """The sphere-placement rule (fingermodel.cpp:208-267, thumbmodel.cpp:227-274), restated:
    segment seg of digit d between joints seg and seg + 1 carries ns spheres at
    (1 - t j) joint_a + (t j) joint_b; a finger's first segment has 4 with t = 1/3 from j = 0
    (both ends), every other segment 2 with t = 1/2 from j = 1 (its far end included)."""
    wa, wb, dg, ja = [], [], [], []
    for d in range(5):
        for seg in range(4):
            if seg == 0 and d != 0:
                t, js = 1.0 / (4 - 1), range(0, 4)
            else:
                t, js = 1.0 / 2, range(1, 3)
            for j in js:
                wa.append(1.0 - t * j)
                wb.append(t * j)
                dg.append(d)
                ja.append(seg)
    return np.array(wa), np.array(wb), np.array(dg, np.int32), np.array(ja, np.int32)


def _ulps(a, b):
    """|a - b| in units of the larger magnitude's ulp (0 where equal, signed zeros included)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.abs(a - b)
    with np.errstate(invalid="ignore"):
        return np.where(d == 0, 0.0, d / np.spacing(np.maximum(np.abs(a), np.abs(b))))


@pytest.mark.parametrize("name", FAMILY)
def test_build_dev_hand_against_the_oracle(oracle, family, dev_family, name):
    geo, rad, cmc, sp = family[name]
    ora, _ = hand_data.family_oracle_hands(oracle, family[name])
    F = np.array(ora.F[:]).reshape(5, 4, 4)
    T10 = np.array(ora.T10[:]).reshape(5, 4, 4)
    h = dev_family[name]
    # the thumb's twist pCMC = nCMC + pi (hpe_oracle.c build_digit); a finger has none
    pc = oracle_np.deg2rad(float(cmc[0])) + oracle_np.PI
    twc = np.array([math.cos(pc), 1.0, 1.0, 1.0, 1.0])
    tws = np.array([math.sin(pc), 0.0, 0.0, 0.0, 0.0])
    want = dict(Fc=F[:, 0, 0], Fs=F[:, 1, 0], FLc=F[:, 0, 3], FLs=F[:, 1, 3],
                T10x=T10[:, 0, 3], T10y=T10[:, 1, 3], twc=twc, tws=tws,
                L=geo.reshape(5, 4), radii=rad)
    wa, wb, dg, ja = _placement()
    want.update(wa=wa, wb=wb)
    # the matrices' other entries say nothing new, but they do say the layout is as read here
    assert np.array_equal(F[:, 0, 1], -F[:, 1, 0]) and np.array_equal(F[:, 1, 1], F[:, 0, 0])
    assert np.array_equal(np.array(ora.spacing[:]), sp.astype(np.float32))
    worst, where = 0.0, None
    for k, v in want.items():
        u = _ulps(h[k], v).max()
        assert np.isfinite(h[k]).all(), k
        if u > worst:
            worst, where = u, k
    print(f"hand {name}: DevHand against the oracle's constants: "
          + ("bit for bit" if worst == 0 else f"at most {worst:.3g} ulp (in {where})"))
    for k, v in want.items():
        assert _ulps(h[k], v).max() <= 4, (k, h[k], v)
    assert np.array_equal(h["dg"], dg) and np.array_equal(h["ja"], ja)
    assert len(wa) == 48
    # the branches: a thumb's T10 is -a (cos, sin) beta, a finger's -L0 sin(n) (cos, sin) beta
    n = oracle_np.deg2rad(cmc.astype(np.float64))
    L0 = geo.reshape(5, 4)[:, 0]
    beta = np.arctan2(h["T10y"], h["T10x"]) - math.pi  # the angle of -(x, y)
    r = np.hypot(h["T10x"], h["T10y"])
    sp32 = sp.astype(np.float32)
    spf, sp2 = sp32.astype(np.float64), (sp32 * sp32).astype(np.float64)  # a float product
    a = np.sqrt(L0 * L0 + sp2 - 2 * L0 * spf * np.cos(n))
    assert abs(r[0] - a[0]) < 1e-12 and np.abs(r[1:] - L0[1:] * np.sin(n[1:])).max() < 1e-12
    # beta has the spacing's sign (0 where the spacing is 0)
    s_beta = np.sin(beta)
    assert np.array_equal(np.sign(np.round(s_beta, 12)), np.sign(spf) * np.sign(np.sin(n)))
