"""CPU-side checks of lane cleaning (hpe_set_batch_clean, hpe_clean_depth_u16,
hpe_batch_clean_readback, hpe_clean_defaults; no GPU):

* hpe_clean's layout in the header and the binding (8 bytes), and the four entry points declared,
  exported and in the signature table; hpe_clean_defaults (host only) equals hpe.clean.defaults;
* hpe.clean.clean, the host side of the rule, has known answers worked out by hand on 5x5
  patches, placed in a frame's interior, at each of its four corners and on each of its four edges
  -- one at a time and all nine at once, so an index that wraps from column 0 to column 319 of
  the row above would count a neighbour that is not one;
* the mirror equals a slow per-pixel restatement of the rule in plain Python on random frames;
* support = 0 without the median is the identity;
* hpe.synth.camera_noise is deterministic, and on its output over a hand-shaped blob the default
  parameters zero more than 90 % of the injected pixels and all but at most 1 % of the hand's
  interior stays non-zero.  Why those bounds: a flying pixel lies 20 % .. 80 % of the way from the
  hand (about 450) to the background (800), at least 70 counts from every hand pixel and so near
  none at edge 15; it is kept only if three of its neighbours are flying pixels within 15 counts of
  it, and two flying depths drawn over 210 counts are that close with probability about 1/7 -- so
  well under a tenth survive.  A speckle pixel lies two or more pixels from the hand and has no
  neighbour unless another speckle pixel landed beside it.  An interior pixel (all eight
  neighbours on the hand, before the noise) loses at most the neighbours that turned into flying
  pixels, and the blob's own depth differs by at most a few counts between neighbours.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import hand_data

NAMES = {"hpe_clean_defaults": 2, "hpe_set_batch_clean": 3, "hpe_clean_depth_u16": 5,
         "hpe_batch_clean_readback": 4}
PKG = hand_data.ROOT / "hand-pose-estimation_amd"
H, W = 240, 320


def _header():
    txt = (hand_data.ROOT / "include" / "hpe.h").read_text()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_struct_layout_and_size():
    from hpe import _lib, clean
    assert C.sizeof(_lib.CleanPar) == 8
    names = [f[0] for f in _lib.CleanPar._fields_]
    assert tuple(names) == clean.FIELDS == ("edge", "support", "flags", "pad")
    assert [getattr(_lib.CleanPar, n).offset for n in names] == [0, 2, 3, 4]
    assert [f[1] for f in _lib.CleanPar._fields_] == [C.c_uint16, C.c_uint8, C.c_uint8, C.c_uint32]
    m = re.search(r"typedef\s+struct\s+hpe_clean\s*\{(.*?)\}\s*hpe_clean\s*;", _header(), flags=re.S)
    assert m, "no hpe_clean in the header"
    decl = re.findall(r"(uint\d+_t)\s+(\w+)\s*;", m.group(1))
    assert decl == [("uint16_t", "edge"), ("uint8_t", "support"), ("uint8_t", "flags"),
                    ("uint32_t", "pad")]
    assert re.search(r"#define\s+HPE_CLEAN_MEDIAN\s+1u", _header())
    assert _lib.CLEAN_MEDIAN == 1 == clean.MEDIAN


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_exported_and_in_the_signature_table(name):
    from hpe import _lib
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, "no declaration"
    assert len(m.group(1).split(",")) == NAMES[name]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libhpe.so")],
                        capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + name + r"$", nm, flags=re.M)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == NAMES[name]
    assert getattr(_lib.load(), name).argtypes == args


def test_defaults_host_only():
    from hpe import _lib, clean
    lib = _lib.load()
    for unit in (1.0, 0.5, 0.0055, 0.1, 2.0, 100.0, 1e-6, 6.0, 10.0):
        out = _lib.CleanPar(9, 9, 9, 9)
        assert lib.hpe_clean_defaults(unit, C.byref(out)) == 0
        want = clean.defaults(unit)
        assert (out.edge, out.support, out.flags, out.pad) == \
            (want.edge, want.support, want.flags, want.pad), unit
        assert 1 <= out.edge <= 65535 and out.support == 3 and out.flags == clean.MEDIAN
    assert clean.defaults(1.0).edge == 15 and clean.defaults(0.5).edge == 30
    assert clean.defaults(100.0).edge == 1 and clean.defaults(1e-6).edge == 65535
    assert clean.defaults(6.0).edge == 2 and clean.defaults(10.0).edge == 2  # 2.5, 1.5: ties to even
    out = _lib.CleanPar()
    for unit in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.hpe_clean_defaults(unit, C.byref(out)) == _lib.HPE_E_ARG
    assert lib.hpe_clean_defaults(1.0, None) == _lib.HPE_E_ARG
    # a null context is refused by the calls that take one
    assert lib.hpe_set_batch_clean(None, 1, C.byref(out)) == _lib.HPE_E_ARG
    assert lib.hpe_clean_depth_u16(None, None, None, None, None) == _lib.HPE_E_ARG
    assert lib.hpe_batch_clean_readback(None, 0, 0, None) == _lib.HPE_E_ARG


# ---- known answers, worked out by hand
# A: an island with a zero rim (edge 10).  Near neighbours s per pixel: 100: {104, 102, 110} 3;
# 104: {100, 102, 110, 108} 4; 300: 0; 102: {100, 104, 110, 106} 4; 110: {100, 104, 102, 108, 106} 5;
# 108: {104, 110, 106} 3; 106: {102, 110, 108} 3; 500: 0.
A = np.array([[0, 0, 0, 0, 0],
              [0, 100, 104, 300, 0],
              [0, 102, 110, 108, 0],
              [0, 0, 106, 0, 0],
              [0, 0, 0, 0, 500]], dtype=np.uint16)
A_S2 = np.array([[0, 0, 0, 0, 0],          # support 2: 300 and 500 go
                 [0, 100, 104, 0, 0],
                 [0, 102, 110, 108, 0],
                 [0, 0, 106, 0, 0],
                 [0, 0, 0, 0, 0]], dtype=np.uint16)
A_S4 = np.array([[0, 0, 0, 0, 0],          # support 4: s >= 4 only
                 [0, 0, 104, 0, 0],
                 [0, 102, 110, 0, 0],
                 [0, 0, 0, 0, 0],
                 [0, 0, 0, 0, 0]], dtype=np.uint16)
# support 2 with the median, sorted C and index s // 2: 100: {100,102,104,110}[1] = 102;
# 104: {100,102,104,108,110}[2] = 104; 102: {100,102,104,106,110}[2] = 104;
# 110: {100,102,104,106,108,110}[2] = 104 (even count: the lower median); 108: {104,106,108,110}[1]
# = 106; 106: {102,106,108,110}[1] = 106
A_S2_MED = np.array([[0, 0, 0, 0, 0],
                     [0, 102, 104, 0, 0],
                     [0, 104, 104, 106, 0],
                     [0, 0, 106, 0, 0],
                     [0, 0, 0, 0, 0]], dtype=np.uint16)
# B: a full block of one value, edge 0, support 5: its corners have 3 near neighbours, its edge
# pixels 5, the inner ones 8 -- wherever it lies, the image's outside reading 0
B = np.full((5, 5), 200, dtype=np.uint16)
B_S5 = B.copy()
B_S5[[0, 0, 4, 4], [0, 4, 0, 4]] = 0
# G: v = 200 + 10 r + c, edge 1: only the left and right neighbours are near (rows differ by 10,
# diagonals by 9 or 11).  support 2 keeps columns 1..3; the median at support 1 gives v in columns
# 0..3 ({v, v+1}[0], {v-1, v, v+1}[1]) and v - 1 in column 4 ({v-1, v}[0])
G = (200 + 10 * np.arange(5)[:, None] + np.arange(5)[None, :]).astype(np.uint16)
G_S2 = G.copy()
G_S2[:, [0, 4]] = 0
G_S1_MED = G.copy()
G_S1_MED[:, 4] -= 1

PLACES = {"interior": (117, 201), "top left": (0, 0), "top right": (0, W - 5),
          "bottom left": (H - 5, 0), "bottom right": (H - 5, W - 5), "top edge": (0, 77),
          "bottom edge": (H - 5, 150), "left edge": (60, 0), "right edge": (171, W - 5)}
CASES = [("A support 2", A, 10, 2, False, A_S2), ("A support 4", A, 10, 4, False, A_S4),
         ("A median", A, 10, 2, True, A_S2_MED), ("B support 5", B, 0, 5, False, B_S5),
         ("B median", B, 0, 5, True, B_S5), ("G support 2", G, 1, 2, False, G_S2),
         ("G median", G, 1, 1, True, G_S1_MED)]


def _placed(patch, places):
    f = np.zeros((H, W), dtype=np.uint16)
    for r, c in places:
        f[r:r + 5, c:c + 5] = patch
    return f


@pytest.mark.parametrize("what,patch,edge,support,median,want", CASES, ids=[c[0] for c in CASES])
def test_known_answers(what, patch, edge, support, median, want):
    from hpe import clean
    for name, at in PLACES.items():
        got = clean.clean(_placed(patch, [at]), edge, support, median)
        assert np.array_equal(got, _placed(want, [at])), (what, name)
    # all nine at once: the patches at the image's two sides do not see each other
    got = clean.clean(_placed(patch, PLACES.values()), edge, support, median)
    assert np.array_equal(got, _placed(want, PLACES.values())), what


def slow_clean(f, edge, support, median):
    """The rule restated pixel by pixel, in plain Python integers."""
    h, w = f.shape
    F = [[int(v) for v in row] for row in f]
    out = [[0] * w for _ in range(h)]
    for r in range(h):
        for c in range(w):
            u = F[r][c]
            if u == 0:
                continue
            near = []
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    if (dr or dc) and 0 <= r + dr < h and 0 <= c + dc < w:
                        q = F[r + dr][c + dc]
                        if q != 0 and abs(q - u) <= edge:
                            near.append(q)
            s = len(near)
            if s < support:
                continue
            out[r][c] = sorted(near + [u])[s // 2] if median else u
    return np.array(out, dtype=np.uint16)


@pytest.mark.parametrize("edge,support,median", [(0, 0, False), (3, 1, True), (40, 3, True),
                                                 (40, 5, False), (65535, 8, True), (1000, 2, True)])
def test_mirror_equals_the_slow_restatement(edge, support, median):
    from hpe import clean
    rng = np.random.default_rng(edge + 7 * support)
    for shape, hi in (((23, 31), 120), ((17, 40), 65536)):
        f = rng.integers(1, hi, size=shape).astype(np.uint16)
        f[rng.random(shape) < 0.3] = 0
        f[0, 0], f[-1, -1] = 65535, 1
        assert np.array_equal(clean.clean(f, edge, support, median),
                              slow_clean(f, edge, support, median))


def test_identity_at_support_0_without_the_median():
    from hpe import clean
    rng = np.random.default_rng(5)
    f = rng.integers(0, 65536, size=(H, W)).astype(np.uint16)
    for edge in (0, 15, 65535):
        got = clean.clean(f, edge, 0, False)
        assert got.dtype == np.uint16 and np.array_equal(got, f) and got is not f
    with pytest.raises(TypeError):
        clean.clean(f.astype(np.int32), 1, 1, False)
    with pytest.raises(ValueError):
        clean.clean(f, 1, 9, False)
    for bad in (clean.Clean(1, 9), clean.Clean(1, 1, 2), clean.Clean(1, 1, 0, 1), clean.Clean(70000, 1)):
        with pytest.raises(ValueError):
            bad.check()
    assert clean.as_clean((15, 3, 1)) == clean.Clean(15, 3, 1, 0) == clean.defaults(1.0)


def blob():
    """A hand-shaped blob at about 450 counts: a palm and four fingers, a smooth depth."""
    r, c = np.mgrid[0:H, 0:W]
    on = ((r - 150) / 40.0) ** 2 + ((c - 160) / 34.0) ** 2 <= 1.0
    for k in range(4):
        on |= (np.abs(c - (133 + 18 * k)) <= 5) & (r >= 60 + 4 * abs(k - 1.5)) & (r <= 130)
    z = 450.0 + 0.08 * (r - 150) + 0.05 * (c - 160)
    return np.where(on, np.rint(z), 0).astype(np.uint16)


def test_camera_noise_and_the_defaults():
    from hpe import clean, synth
    f = blob()
    on = f > 0
    a = synth.camera_noise(f, 11)
    assert np.array_equal(a, synth.camera_noise(f, 11)) and a.dtype == np.uint16  # deterministic
    assert not np.array_equal(a, synth.camera_noise(f, 12)) and np.array_equal(f, blob())
    injected = a != f
    flying, speckle = injected & on, injected & ~on
    assert flying.sum() >= 100 and speckle.sum() == 40
    assert (a[flying] > f[flying] + 60).all() and (a[flying] < 800).all()
    assert (np.abs(a[speckle].astype(int) - 450) <= 40).all()
    p = clean.defaults(1.0)
    got = p.apply(a)
    zeroed = int((got[injected] == 0).sum())
    print(f"injected {int(injected.sum())}, zeroed {zeroed}")
    assert zeroed > 0.9 * injected.sum()
    # the interior: every neighbour on the hand
    pad = np.zeros((H + 2, W + 2), dtype=bool)
    pad[1:-1, 1:-1] = on
    interior = on.copy()
    for dr in range(3):
        for dc in range(3):
            interior &= pad[dr:dr + H, dc:dc + W]
    lost = int((got[interior] == 0).sum())
    print(f"interior {int(interior.sum())}, lost {lost}")
    assert interior.sum() > 5000 and lost <= 0.01 * interior.sum()
    # and what is kept there stays within the edge of what was rendered
    kept = interior & (got != 0)
    assert (np.abs(got[kept].astype(int) - f[kept].astype(int)) <= p.edge).all()
