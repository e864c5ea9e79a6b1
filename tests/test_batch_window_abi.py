"""CPU-side checks of the lane windows (hpe_set_batch_window, hpe_window_from_pose,
hpe_batch_windows_readback; no GPU):

* the three entry points are declared in include/hpe.h, exported by libhpe.so and in the
  binding's signature table; HPE_WINDOW_OFF / _FIXED / _FOLLOW are 0 / 1 / 2 in both; the
  binding's struct has hpe_window's 32 bytes; a null context is refused with HPE_E_ARG;
* known answers of the host mirror hpe.window: `apply` (the masking rule -- inclusive bounds, the
  depth test on rv / 10, the whole-frame window, an empty window) and `from_spheres` (the pose
  rule on exactly representable numbers, the clamps, the fail-open cases).
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import hand_data

NAMES = {"hpe_set_batch_window": 6, "hpe_window_from_pose": 6, "hpe_batch_windows_readback": 4}
PKG = hand_data.ROOT / "hand-pose-estimation_amd"
INF = float("inf")


def _header():
    txt = (hand_data.ROOT / "include" / "hpe.h").read_text()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


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
    assert len(args) == NAMES[name]
    assert getattr(_lib.load(), name).argtypes == args


def test_constants_and_struct_size():
    from hpe import _lib
    import hpe
    txt = _header()
    for name, val in (("OFF", 0), ("FIXED", 1), ("FOLLOW", 2)):
        assert re.search(r"#define\s+HPE_WINDOW_%s\s+%d\b" % (name, val), txt)
        assert getattr(_lib, "WINDOW_" + name) == val
        assert hpe.WINDOW_MODES[name.lower()] == val
    assert C.sizeof(_lib.Window) == 32
    assert _lib.Window.z_lo.offset == 16 and _lib.Window.z_hi.offset == 24
    assert re.search(r"typedef\s+struct\s+hpe_window\s*\{[^}]*int32_t\s+row_lo,\s*row_hi,\s*col_lo,"
                     r"\s*col_hi;[^}]*double\s+z_lo,\s*z_hi;[^}]*\}\s*hpe_window;", txt)


def test_null_context_is_refused():
    from hpe import _lib
    lib = _lib.load()
    w = (_lib.Window * 1)()
    th = np.zeros(26)
    assert lib.hpe_set_batch_window(None, 0, 1, None, 0.0, 0.0) == _lib.HPE_E_ARG
    assert lib.hpe_set_batch_window(None, 1, 1, w, 1.0, 1.0) == _lib.HPE_E_ARG
    assert lib.hpe_window_from_pose(None, th.ctypes.data_as(_lib.dp), 241.42, 1.0, 1.0, w) == _lib.HPE_E_ARG
    assert lib.hpe_batch_windows_readback(None, 0, 1, w) == _lib.HPE_E_ARG


def test_python_side_argument_checks():
    import hpe
    ctx = object.__new__(hpe.Context)  # never reached hpe_create
    with pytest.raises(ValueError):
        ctx.set_batch_window("sometimes")
    with pytest.raises(ValueError):
        ctx.set_batch_window("fixed", [(0, 1, 2)])


# ---- hpe.window.apply: the masking rule
def _frame():
    """Raw value 10 (r + 1) + c / 32 mm at (r, c): every pixel non-zero and distinct per row."""
    r = np.arange(240, dtype=np.float32)[:, None]
    c = np.arange(320, dtype=np.float32)[None, :]
    return (10 * (r + 1) + c / 32).astype(np.float32)


def test_apply_inclusive_bounds():
    from hpe import window
    d = _frame()
    out = window.apply(d, (3, 5, 7, 11, -INF, INF))
    assert out.dtype == np.float32 and out.shape == (240, 320)
    want = np.zeros_like(d)
    want[3:6, 7:12] = d[3:6, 7:12]
    assert np.array_equal(out, want)
    assert np.count_nonzero(out) == 3 * 5
    # a one-pixel window, and the image corners
    assert np.count_nonzero(window.apply(d, (239, 239, 319, 319, -INF, INF))) == 1
    assert window.apply(d, (0, 0, 0, 0, -INF, INF))[0, 0] == d[0, 0]


def test_apply_depth_test_is_on_rv_over_10():
    from hpe import window
    d = np.zeros((240, 320), np.float32)
    d[0, :5] = (299.0, 300.0, 305.0, 310.0, 311.0)  # Z = 29.9, 30, 30.5, 31, 31.1 cm
    out = window.apply(d, (0, 239, 0, 319, 30.0, 31.0))
    assert np.array_equal(out[0, :5], np.array((0, 300.0, 305.0, 310.0, 0), np.float32))
    # without to_cm the bounds are in the raw unit
    out = window.apply(d, (0, 239, 0, 319, 300.0, 310.0), to_cm=False)
    assert np.array_equal(out[0, :5], np.array((0, 300.0, 305.0, 310.0, 0), np.float32))
    # Z is the fp64 quotient of the fp32 value: 300.1f / 10. lies above 30.01 rounded to fp64?
    rv = np.float32(300.1)
    z = float(rv) / 10.
    d[1, 0] = rv
    assert window.apply(d, (1, 1, 0, 0, z, z))[1, 0] == rv
    assert window.apply(d, (1, 1, 0, 0, np.nextafter(z, INF), INF))[1, 0] == 0


def test_apply_whole_and_empty_windows():
    from hpe import window
    d = _frame()
    d[17, 40:60] = 0.0
    assert np.array_equal(window.apply(d, window.WHOLE), d)
    assert np.array_equal(window.apply(d, (0, 239, 0, 319, -INF, INF)), d)
    assert window.is_whole((0, 239, 0, 319, -INF, INF)) and not window.is_whole((0, 239, 0, 318, -INF, INF))
    zero = np.zeros_like(d)
    for w in (window.EMPTY, (5, 4, 0, 319, -INF, INF), (0, 239, 9, 8, -INF, INF),
              (0, 239, 0, 319, 2.0, 1.0), (0, 239, 0, 319, float("nan"), INF),
              (0, 239, 0, 319, -INF, float("nan"))):
        assert np.array_equal(window.apply(d, w), zero), w


def test_apply_takes_the_binding_struct():
    from hpe import _lib, window
    d = _frame()
    w = _lib.Window(3, 5, 7, 11, -INF, INF)
    assert np.array_equal(window.apply(d, w), window.apply(d, (3, 5, 7, 11, -INF, INF)))


# ---- hpe.window.from_spheres: the pose rule
def _S(cam):
    """Centres as hpe_build_spheres returns them (y and z negated) from camera coordinates."""
    s = np.array(cam, dtype=np.float64).reshape(-1, 3).copy()
    s[:, 1:3] *= -1
    return s


def test_from_spheres_known_answer():
    from hpe import window
    w = window.from_spheres(_S([(0, 0, 32)]), [1.0], 240.0, 1.0, 2.0)
    assert w == window.Window(105, 135, 145, 175, 29.0, 35.0)
    assert all(isinstance(v, int) for v in w[:4]) and all(isinstance(v, float) for v in w[4:])
    # two centres: minima and maxima over both; floor, not truncation, below zero
    w = window.from_spheres(_S([(0, 0, 32), (8, -4, 16)]), [1.0, 2.0], 240.0, 1.0, 2.0)
    # second: e = 3; cl = (240*5 + 2560)/16 = 235, ch = (240*11 + 2560)/16 = 325 -> 319;
    #         rl = (240*-7 + 1920)/16 = 15, rh = (240*-1 + 1920)/16 = 105; z 12..20
    assert w == window.Window(15, 135, 145, 319, 12.0, 35.0)
    w = window.from_spheres(_S([(-24, 0, 32)]), [1.0], 240.5, 1.0, 0.0)
    # cl = floor((240.5*-26 + 5120)/32) = floor(-35.40625) = -36 -> 0; ch = floor(-5.34375) = -6 -> -1
    assert (w.col_lo, w.col_hi) == (0, -1)


def test_from_spheres_clamps():
    from hpe import window
    # far right and below: lo clamps to 320 / 240 (an empty window), hi to 319 / 239
    w = window.from_spheres(_S([(64, 64, 32)]), [1.0], 240.0, 1.0, 0.0)
    assert w[:4] == (239 + 1, 239, 319 + 1, 319)
    assert not window.keep_mask(np.ones((240, 320), np.float32), w).any()
    # far left and above: hi clamps to -1, lo to 0
    w = window.from_spheres(_S([(-64, -64, 32)]), [1.0], 240.0, 1.0, 0.0)
    assert w[:4] == (0, -1, 0, -1)
    # huge margin: the whole image, a finite depth range
    w = window.from_spheres(_S([(0, 0, 32)]), [1.0], 240.0, 1000.0, 5.0)
    assert w == window.Window(0, 239, 0, 319, 26.0, 38.0)


@pytest.mark.parametrize("bad", [(float("nan"), 0, 32), (0, float("inf"), 32), (0, 0, float("nan")),
                                 (0, 0, 0.0), (0, 0, -32.0), (0, 0, float("inf"))])
def test_from_spheres_fails_open(bad):
    from hpe import window
    w = window.from_spheres(_S([(0, 0, 32), bad, (1, 1, 30)]), [1.0, 1.0, 1.0], 240.0, 1.0, 2.0)
    assert w == window.Window(0, 239, 0, 319, -INF, INF)
    assert window.is_whole(w)
