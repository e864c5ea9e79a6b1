"""hpe_locate_depth, the location rule on the device, against its numpy mirror hpe/locate.py:
every field of the result np.array_equal, the doubles bit for bit -- nothing here carries a
tolerance.  The frames are the smallest that reach each branch of the rule: the empty frame, one
pixel, one bin holding all 76 800 pixels (counts past 65 535), the last bin and its clamp, depths
on bin edges, the two ends of `skip`, pixels that are not depths, 16-bit values above 32 767 with
a fractional unit, raw millimetres (to_cm = 0), search bounds that are met exactly, and the
rendered hand with its forearm, wall and speckle.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOCAL = 241.42


@pytest.fixture(scope="module")
def ctx():
    import hpe
    hand = hpe.reference_hand(device=0)
    yield hand.ctx
    hand.ctx.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    assert np.array_equal([got.found, got.k_near, got.m1, got.m2], [want.found, want.k_near, want.m1, want.m2]), (got, want)
    assert np.array_equal(bits(got.px), bits(want.px)), (got, want)
    assert np.array_equal(bits(got.centre), bits(want.centre)), (got, want)
    assert np.array_equal(got.window[:4], want.window[:4]), (got, want)
    assert np.array_equal(bits(got.window[4:]), bits(want.window[4:])), (got, want)


def check(ctx, depth, params=None, to_cm=True, unit_mm=None, focal=FOCAL):
    from hpe import locate
    want = locate.locate(depth, focal, locate.DEFAULTS if params is None else params, to_cm, unit_mm)
    got = ctx.locate_depth(depth, focal, params, to_cm, unit_mm)
    same(got, want)
    return want


def both(ctx, mm, params=None, to_cm=True):
    """A frame of whole millimetres in both formats: float, and 16-bit with unit 1."""
    mm = np.asarray(mm, dtype=np.float32)
    assert np.array_equal(mm, np.floor(mm)) and mm.min() >= 0 and mm.max() <= 65535
    a = check(ctx, mm, params, to_cm)
    b = check(ctx, mm.astype(np.uint16), params, to_cm, unit_mm=1.0)
    assert a == b
    return a


def zeros():
    return np.zeros((240, 320), np.float32)


def test_empty_frame(ctx):
    assert both(ctx, zeros()).found == 0


def test_single_valid_pixel(ctx):
    from hpe import locate
    d = zeros()
    d[239, 319] = 612.0
    assert both(ctx, d).found == 0  # one pixel does not pass skip = 20
    r = both(ctx, d, locate.DEFAULTS._replace(skip=0, min_pixels=1))
    assert (r.found, r.m1, r.m2, r.px) == (1, 1, 1, (319.0, 239.0))
    assert both(ctx, d, locate.DEFAULTS._replace(skip=0)).found == 0  # ... nor min_pixels = 200


def test_every_pixel_in_one_bin(ctx):
    from hpe import locate
    full = np.full((240, 320), 400.0, np.float32)
    r = both(ctx, full)
    assert (r.found, r.k_near, r.m1, r.m2) == (1, 80, 76800, 132 * 132)
    r = both(ctx, full, locate.DEFAULTS._replace(half_xy=60.0))  # a box as large as the image
    assert (r.m1, r.m2) == (76800, 76800) and r.px == (159.5, 119.5)


def test_last_bin_and_its_clamp(ctx):
    """K - 1 = 2047 is Z >= 1023.5 cm at bin 0.5: depths just below, at and far beyond it."""
    from hpe import locate
    d = zeros()
    d[10:30, 10:60] = 10230.0   # bin 2046
    d[40:60, 10:60] = 10235.0   # bin 2047 exactly
    d[70:90, 10:60] = 60000.0   # clamped
    p = locate.DEFAULTS._replace(half_xy=500.0, half_z=6000.0)
    r = both(ctx, d, p)
    assert (r.found, r.k_near, r.m1) == (1, 2046, 3000)
    d[10:30, 10:60] = 0.0
    r = both(ctx, d, p)
    assert (r.k_near, r.m1) == (2047, 2000) and r.centre[2] == 2047.5 * 0.5
    f = d.copy()
    f[100:120, 100:160] = np.float32(3.0e38)  # a float far beyond every bin: clamped, not wrapped
    r = check(ctx, f, p)
    assert (r.k_near, r.m1) == (2047, 3200)
    u = np.full((240, 320), 65535, np.uint16)
    assert check(ctx, u, p, unit_mm=1.0).k_near == 2047


@pytest.mark.parametrize("bin_", [0.5, 0.1, 0.3])
def test_depths_on_bin_edges(ctx, bin_):
    """A ramp of quarter millimetres over the frame: hundreds of depths that are a whole number of
    bins, or one float away from it, under a bin that fp64 does and does not represent."""
    from hpe import locate
    i = np.arange(76800, dtype=np.float64).reshape(240, 320)
    d = (300.0 + (i % 1600) * 0.25).astype(np.float32)
    p = locate.DEFAULTS._replace(bin=bin_, min_pixels=1)
    check(ctx, d, p)
    check(ctx, np.nextafter(d, np.float32(0)), p)
    check(ctx, np.nextafter(d, np.float32(1e9)), p, to_cm=False)
    u = (1200 + (i % 1600)).astype(np.uint16)
    check(ctx, u, p, unit_mm=0.25)


def test_skip_at_both_ends(ctx):
    from hpe import locate
    d = zeros()
    d[100:120, 100:130] = 400.0  # 600 valid pixels
    d[50, 50] = 90.0
    assert both(ctx, d, locate.DEFAULTS._replace(skip=0)).k_near == 18
    assert both(ctx, d, locate.DEFAULTS._replace(skip=1)).k_near == 80
    assert both(ctx, d, locate.DEFAULTS._replace(skip=600)).k_near == 80
    for skip in (601, 602, 76800, 2 ** 31 - 1):  # skip >= the valid count
        r = both(ctx, d, locate.DEFAULTS._replace(skip=skip))
        assert (r.found, r.k_near, r.m1, r.m2) == (0, -1, 0, 0)


def test_pixels_that_are_not_depths(ctx):
    from hpe import locate
    d = zeros()
    d[100:120, 100:130] = 400.0
    d[0, :] = np.nan
    d[1, :] = np.inf
    d[2, :] = -np.inf
    d[3, :] = -250.0
    d[4, :] = -0.0
    clean = zeros()
    clean[100:120, 100:130] = 400.0
    r = check(ctx, d, locate.DEFAULTS._replace(skip=0))
    assert r == locate.locate(clean, FOCAL, locate.DEFAULTS._replace(skip=0)) and r.m1 == 600


def test_u16_above_32767_with_a_fractional_unit(ctx):
    from hpe import locate
    u = np.zeros((240, 320), np.uint16)
    u[60:100, 200:260] = 40000
    u[61, 201] = 65535
    u[10:14, 10:14] = 32768
    for unit in (0.01, 0.3, 1.0 / 3.0, 0.125):
        r = check(ctx, u, locate.DEFAULTS._replace(skip=0, min_pixels=1), unit_mm=unit)
        # 32768 counts are the nearest object; at 1/3 mm it lies beyond the last bin, whose
        # depth the box then misses
        assert r.m1 > 0 and r.found == (0 if unit == 1.0 / 3.0 else 1)
        check(ctx, u, unit_mm=unit)


def test_raw_millimetres(ctx):
    """to_cm = 0: Z is the raw value, and the parameters are millimetres."""
    from hpe import locate
    d = zeros()
    d[100:140, 150:200] = 400.0
    p = locate.DEFAULTS._replace(bin=5.0, slab=120.0, half_xy=110.0, half_z=110.0)
    r = both(ctx, d, p, to_cm=False)
    assert (r.found, r.k_near, r.m1, r.centre[2]) == (1, 80, 2000, 402.5)
    assert both(ctx, d, to_cm=False).k_near == 800  # the cm defaults on mm: bin 0.5 mm


def test_inclusive_search_edges(ctx):
    from hpe import locate, window
    d = zeros()
    d[100:140, 150:200] = 400.0
    d[99, 150:200] = 300.0    # one row, one column and one depth outside each bound
    d[100:140, 149] = 300.0
    for s, m in ((window.Window(100, 139, 150, 199, 40.0, 40.0), 2000),   # met exactly
                 (window.Window(101, 138, 151, 198, 40.0, 40.0), 38 * 48),
                 (window.Window(99, 139, 149, 199, 40.0, 40.0), 2000),   # the 300 mm pixels: depth
                 (window.Window(99, 139, 149, 199, 30.0, 40.0), 2090),
                 (window.Window(100, 139, 150, 199, np.nextafter(40.0, 41.0), 50.0), 0),
                 (window.Window(100, 139, 150, 199, 30.0, np.nextafter(40.0, 39.0)), 0),
                 (window.Window(139, 100, 150, 199, 0.0, 99.0), 0),        # lo > hi keeps nothing
                 (window.Window(0, 239, 0, 319, np.nan, 99.0), 0)):        # ... and so does NaN
        r = both(ctx, d, locate.DEFAULTS._replace(search=s, skip=0, slab=20.0, min_pixels=1))
        assert r.m1 == m, (s, r)
        assert r.found == (1 if m else 0)


def test_hand_arm_and_wall_scene(ctx):
    import hpe
    from hpe import synth, window
    for th in (np.asarray(hpe.X0, dtype=np.float64), synth.trajectory(25)[8]):
        hand = ctx.render_depth(th)
        scene = synth.rig_scene(hand, th[3:6], FOCAL)
        r = check(ctx, scene)
        assert r.found == 1
        keep = window.keep_mask(scene, r.window)
        assert (keep & (hand > 0)).sum() == (hand > 0).sum() and (keep & (scene == 800.0)).sum() == 0
        q = np.round(scene / np.float32(0.25)).astype(np.uint16)
        assert check(ctx, q, unit_mm=0.25).found == 1


def test_refusals(ctx):
    from hpe import _lib, locate
    lib, h = ctx.lib, ctx.h
    d = zeros()
    r = _lib.Locate()

    def call(frame=d.ctypes.data, u16=0, unit=1.0, focal=FOCAL, out=C.byref(r), **kw):
        p = ctx._locate_params(locate.DEFAULTS._replace(**kw))
        return lib.hpe_locate_depth(h, frame, u16, unit, 1, focal, C.byref(p), out)

    assert call() == 0
    assert call(frame=None) == _lib.HPE_E_ARG and call(out=None) == _lib.HPE_E_ARG
    for kw in (dict(bin=0.0), dict(bin=-1.0), dict(bin=np.nan), dict(bin=np.inf), dict(slab=-1.0),
               dict(slab=np.inf), dict(half_xy=-0.5), dict(half_xy=np.nan), dict(half_z=-1.0),
               dict(half_z=np.inf), dict(skip=-1), dict(min_pixels=-1)):
        assert call(**kw) == _lib.HPE_E_ARG, kw
    assert call(focal=0.0) == _lib.HPE_E_ARG and call(focal=np.nan) == _lib.HPE_E_ARG
    assert call(u16=1, unit=0.0) == _lib.HPE_E_ARG and call(u16=1, unit=np.inf) == _lib.HPE_E_ARG
    assert lib.hpe_locate_depth(h, d.ctypes.data, 0, 1.0, 1, FOCAL, None, C.byref(r)) == 0  # defaults
