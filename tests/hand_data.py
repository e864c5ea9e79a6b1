"""Reference hand geometry (misc/hgeo.dat, misc/rad.dat values, committed as package
data) and synthetic frame helpers shared by the tests."""
import json
import os
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
HAND_JSON = ROOT / "hand-pose-estimation_amd" / "hpe" / "hand_subject1.json"

# The GPU contexts' refine form (hpe_create reads HPE_REFINE_EXACT): the hand-frame refine
# by default, compared with the oracle's mirror of it; the reference's chain under
# HPE_REFINE_EXACT=1, compared with the oracle's restatement (tests/test_rigid.py bounds
# the distance between the two).
REFINE_RIGID = os.environ.get("HPE_REFINE_EXACT", "0") != "1"


def geometry_cm():
    d = json.loads(HAND_JSON.read_text())
    return np.array(d["hgeo_mm"]) / 10.0, np.array(d["rad_mm"]) / 10.0


FAMILY = ("ref", "V", "small", "large", "uneven", "mirror", "zero_sp", "right_angle")


def hand_family():
    """{name: (geo_cm (20,), radii_cm (48,), cmc_deg (5,), spacing_cm (5,))}: the hands that the
    oracle comparisons of tests/test_hand_family.py and tests/test_gpu_hand_family.py run on.
    The reference hand hides the branches the others reach: a middle finger whose spacing is not
    0 (uneven), spacings of the other sign (mirror) and all 0 (zero_sp), CMC angles at and across
    90 degrees (right_angle, uneven), lengths and radii that are no common multiple of the
    reference's (uneven), and V, the hand of tests/test_gpu_batch_hands.py."""
    import oracle_np
    geo, rad = geometry_cm()
    cmc, sp = np.array(oracle_np.CMC), np.array(oracle_np.SPACING)
    return {
        "ref": (geo, rad, cmc, sp),
        "V": (geo * 1.05, rad * 0.95, cmc + np.array([1.5, -1.0, 0.5, 0.75, -0.5]),
              sp + np.array([0.05, -0.04, 0.03, 0.02, -0.06])),
        "small": (geo * 0.7, rad * 0.7, cmc, sp * 0.7),
        "large": (geo * 1.3, rad * 1.25, cmc, sp * 1.3),
        "uneven": (geo * np.repeat((1.2, 0.8, 1.1, 0.9, 1.15), 4) * np.tile((1, 0.9, 1.1, 1.2), 5),
                   rad * np.linspace(0.8, 1.3, 48), cmc + np.array([-12.0, 9, -7, 6, 11]),
                   sp + np.array([0.4, -0.3, 0.5, -0.6, 0.7])),
        "mirror": (geo, rad, cmc, -sp),
        "zero_sp": (geo, rad, cmc, np.zeros(5)),
        "right_angle": (geo, rad, np.array([150.0, 90, 90, 90, 45]), sp),
    }


def family_gpu_hand(entry, params_only=False):
    """A family entry as hpe.handmodel (a context of its own) or, params_only, as the
    hpe._lib.HandParams that hpe_set_batch_hands takes (no context)."""
    import hpe
    geo, rad, cmc, sp = entry
    if not params_only:
        return hpe.handmodel(geo, sp, hpe.TB_SPHERES, hpe.FG_SPHERES, cmc, rad)
    p = hpe._lib.HandParams()
    p.geo_cm[:] = [float(x) for x in geo]
    p.radii_cm[:] = [float(x) for x in rad]
    p.cmc_deg[:] = [float(x) for x in cmc]
    p.spacing_cm[:] = [float(x) for x in sp]
    p.tb_spheres[:] = hpe.TB_SPHERES
    p.fg_spheres[:] = hpe.FG_SPHERES
    return p


def family_oracle_hands(oracle, entry):
    """A family entry as (C oracle hand, numpy oracle hand)."""
    import oracle_np
    geo, rad, cmc, sp = entry
    return oracle.hand(geo, rad, cmc, sp), oracle_np.Hand(geo, rad, cmc, sp)


def family_poses():
    """The FK poses of the family tests: X0, the zero pose, a global rotation of (180, -180, 90),
    the lower and the upper bound, and 12 seeded draws of spread 3 (17 x 26)."""
    import oracle_np
    ub, lb, _ = oracle_np.reference_bounds()
    turned = oracle_np.X0.copy()
    turned[0:3] = (180.0, -180.0, 90.0)
    return np.vstack([oracle_np.X0, np.zeros(26), turned, lb, ub,
                      random_thetas(np.random.default_rng(77), 12, spread=3.0)])


# csrc/hpe_layout.hpp's DevHand as tests/cpp/dev_hand_dump.cpp writes it (2016 bytes)
DEV_HAND = np.dtype([("Fc", "f8", 5), ("Fs", "f8", 5), ("FLc", "f8", 5), ("FLs", "f8", 5),
                     ("T10x", "f8", 5), ("T10y", "f8", 5), ("L", "f8", (5, 4)), ("twc", "f8", 5),
                     ("tws", "f8", 5), ("radii", "f8", 48), ("wa", "f8", 48), ("wb", "f8", 48),
                     ("dg", "i4", 48), ("ja", "i4", 48)])
_dump_exe = []


def dev_hand_dump(tmp_dir, params):
    """hpe::build_dev_hand of every hpe._lib.HandParams in params, on the host alone: a
    stand-alone program over tests/cpp/dev_hand_dump.cpp and csrc/hpe_host.cpp, built once per
    session into tmp_dir (a pathlib.Path).  Returns (a DEV_HAND array, the program's stdout)."""
    import subprocess
    if not _dump_exe:
        csrc = ROOT / "hand-pose-estimation_amd" / "csrc"
        exe = tmp_dir / "dev_hand_dump"
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", str(exe),
                        str(ROOT / "tests" / "cpp" / "dev_hand_dump.cpp"),
                        str(csrc / "hpe_host.cpp"), f"-I{csrc}"], check=True, timeout=120)
        _dump_exe.append(exe)
    (tmp_dir / "in.bin").write_bytes(b"".join(bytes(p) for p in params))
    out = subprocess.run([str(_dump_exe[0]), str(tmp_dir / "in.bin"), str(tmp_dir / "out.bin")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return np.fromfile(tmp_dir / "out.bin", dtype=DEV_HAND), out.stdout


def random_thetas(rng, P, x0=None, spread=1.0):
    import oracle_np
    x0 = oracle_np.X0 if x0 is None else x0
    ub, lb, sd = oracle_np.reference_bounds()
    th = x0[None, :] + rng.standard_normal((P, 26)) * sd[None, :] * spread
    return np.clip(th, lb, ub)


def trajectory(n_frames, seed=0, revert=0.0):
    """Smooth seeded pose sequence starting at testmodel.cpp's x0;
    revert > 0 pulls the pose back towards x0 so that long sequences stay in view."""
    import oracle_np
    rng = np.random.default_rng(seed)
    ub, lb, sd = oracle_np.reference_bounds()
    poses = [oracle_np.X0.copy()]
    vel = np.zeros(26)
    for _ in range(n_frames - 1):
        vel = 0.8 * vel + 0.2 * rng.standard_normal(26) * sd * 0.15
        vel += revert * (oracle_np.X0 - poses[-1])
        poses.append(np.clip(poses[-1] + vel, lb, ub))
    return np.array(poses)


# (radius scale, spread, seed) of the self-collision cases.  Four of them (scale 1.5 and the
# spread-3 pose of scale 4) are a greedy cover in which each of the 144 sphere pairs is active
# in one case and inactive in another: spread 6 is there for the pair of the middle and ring
# fingers' base spheres, which scale 1.5 separates only in a splayed hand.  Their alignment
# terms are huge, so three poses near the centre follow for each of the scales 2, 3 and 4, in
# which the collision term is at least 12 % of the cost on the frame rendered at the centre
# (tests/test_collision_pairs.py asserts the cover, tests/test_gpu_collision.py the share).
COLLISION_CENTRE = (3, 5, 2)  # trajectory(3, seed=5)[2]
COLLISION_CASES = (
    (1.5, 0.4, 1000), (1.5, 6.0, 1011), (1.5, 6.0, 1037),
    (2.0, 0.4, 1007), (2.0, 0.4, 1016), (2.0, 0.4, 1027),
    (3.0, 0.4, 1000), (3.0, 1.0, 1007), (3.0, 1.0, 1027),
    (4.0, 0.4, 1000), (4.0, 1.0, 1020), (4.0, 1.0, 1039), (4.0, 3.0, 1038),
)


def collision_centre():
    n, seed, k = COLLISION_CENTRE
    return trajectory(n, seed=seed)[k]


def collision_cases():
    """[(radius_scale, theta), ...]: fat-sphere hands (the reference radii times radius_scale,
    as hpe.scaled_hand(1.0, radius_scale)) in seeded poses around collision_centre()."""
    centre = collision_centre()
    return [(k, random_thetas(np.random.default_rng(seed), 1, x0=centre, spread=spread)[0])
            for k, spread, seed in COLLISION_CASES]


def tie_replay(oracle, ora_hand, obs, x0, evals, rigid, tie, pose=None, depth=2):
    """Explain a refine that took `evals` evaluations where the oracle's run from x0 took
    another number: replay the oracle with near-tie decisions (relative margin < tie)
    inverted -- one, then pairs (the second chosen among the flipped run's own later
    near-ties) -- until a replay takes exactly `evals` evaluations (and, if given, reaches
    `pose` within 1e-6).  Returns [(decision, margin), ...] of the flips, or None when no
    combination of near-ties explains it (a real divergence)."""
    import numpy as np

    def run(fl):
        return oracle.refine_log(ora_hand, obs, x0, rigid=rigid, flips=fl)

    _, _, m = run(())
    frontier = [((), (), m)]
    for _ in range(depth):
        nxt = []
        for fl, ms, mm in frontier:
            start = fl[-1] + 1 if fl else 0
            for k in np.flatnonzero(mm < tie):
                if k < start:
                    continue
                f2, m2 = fl + (int(k),), ms + (float(mm[k]),)
                xf, ef, mf = run(f2)
                if ef == evals and (pose is None or np.max(np.abs(xf - pose)) < 1e-6):
                    return list(zip(f2, m2))
                nxt.append((f2, m2, mf))
        frontier = nxt
    return None
