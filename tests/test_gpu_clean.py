"""The cleaning kernel on one frame: hpe_clean_depth_u16 (k_clean_b through a staging buffer)
against hpe.clean.clean, the numpy mirror, with np.array_equal.  Each case is one 240x320 frame,
or one camera frame read through a view, with every camera pixel outside the picks poisoned as
tests/test_gpu_batch_view.py's embed does.  One context runs every case.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_batch_view import embed

pytestmark = pytest.mark.gpu

H, W = 240, 320


@pytest.fixture(scope="module")
def ctx():
    import hpe
    hand = hpe.reference_hand(device=0)
    yield hand.ctx
    hand.ctx.close()


def check(ctx, frame, edge, support, median, view=None):
    from hpe import clean
    p = clean.Clean(edge, support, clean.MEDIAN if median else 0)
    got = ctx.clean_depth_u16(frame, p, view)
    model = frame if view is None else view.reduce(frame)
    want = clean.clean(model, edge, support, median)
    assert got.dtype == np.uint16 and got.shape == (H, W)
    assert np.array_equal(got, want), (edge, support, median, np.argwhere(got != want)[:4])
    return got


def test_all_zero_frame(ctx):
    for median in (False, True):
        assert not check(ctx, np.zeros((H, W), np.uint16), 15, 0, median).any()


@pytest.mark.parametrize("at", [(100, 100), (0, 0), (239, 319), (7, 0), (8, 319)])
def test_one_pixel(ctx, at):
    f = np.zeros((H, W), np.uint16)
    f[at] = 700
    for median in (False, True):
        got = check(ctx, f, 15, 0, median)
        assert got[at] == 700 and np.count_nonzero(got) == 1
        assert not check(ctx, f, 15, 1, median).any()


def test_full_frame_of_one_value_at_support_8(ctx):
    f = np.full((H, W), 1234, np.uint16)
    for median in (False, True):
        got = check(ctx, f, 0, 8, median)
        want = np.zeros_like(f)
        want[1:-1, 1:-1] = 1234  # only the border rows and columns go
        assert np.array_equal(got, want)


def test_difference_of_exactly_edge_and_edge_plus_one(ctx):
    f = np.zeros((H, W), np.uint16)
    f[50, 50], f[50, 51] = 1000, 1020    # exactly edge: near each other
    f[60, 50], f[61, 51] = 1000, 1021    # edge + 1: not near
    f[70, 50], f[71, 49] = 1020, 1000    # exactly edge, the other sign
    got = check(ctx, f, 20, 1, False)
    assert got[50, 50] == 1000 and got[50, 51] == 1020 and got[70, 50] == 1020 and got[71, 49] == 1000
    assert got[60, 50] == 0 and got[61, 51] == 0
    check(ctx, f, 20, 1, True)
    check(ctx, f, 21, 1, False)
    check(ctx, f, 0, 1, False)


def test_16_bit_wrap_of_the_difference(ctx):
    # 65535 - 1 = 65534 is -2 in 16 bits, 32768 - 1 = 32767, 65535 - 32768 = 32767: no pair is near
    f = np.zeros((H, W), np.uint16)
    f[100, 100:103] = [65535, 32768, 1]
    f[110:113, 100] = [1, 65535, 32768]
    for edge in (2, 3, 100, 32766):
        assert not check(ctx, f, edge, 1, False).any()
    got = check(ctx, f, 32767, 1, True)
    assert got.any()
    check(ctx, f, 32767, 2, False)
    check(ctx, f, 65534, 3, True)


def test_edge_65535(ctx):
    rng = np.random.default_rng(3)
    f = rng.integers(0, 65536, size=(H, W)).astype(np.uint16)
    f[rng.random((H, W)) < 0.4] = 0
    for support, median in ((0, True), (4, False), (8, True)):
        check(ctx, f, 65535, support, median)


def test_median_with_ties_and_with_an_even_count(ctx):
    f = np.zeros((H, W), np.uint16)
    f[30:33, 30:33] = [[5, 5, 9], [5, 7, 9], [9, 9, 5]]   # nine values: 5 5 5 5 7 9 9 9 9 -> 7
    f[40:42, 40:43] = [[10, 20, 30], [0, 20, 10]]         # at (40, 41): 10 10 20 20 30, and pairs
    f[50, 50:52] = [100, 104]                             # two values: the lower one
    f[60:62, 60:62] = [[8, 6], [4, 2]]                    # four values: index 1
    got = check(ctx, f, 100, 1, True)
    assert got[31, 31] == 7 and got[30, 30] == 5 and got[40, 41] == 20
    assert got[50, 50] == 100 and got[50, 51] == 100
    assert (got[60:62, 60:62] == 4).all()


def test_random_frame_with_holes(ctx):
    """About 30 % holes, values close enough that near and not near both occur.  The kernel's
    tiles are 8 rows: rows 7|8, 15|16, ..., 231|232 border a tile (the halo rows), and rows 0 and
    239 border the image; every one of them holds kept, zeroed and changed pixels here
    (asserted)."""
    rng = np.random.default_rng(9)
    f = rng.integers(400, 460, size=(H, W)).astype(np.uint16)
    f[rng.random((H, W)) < 0.3] = 0
    assert 0.25 < (f == 0).mean() < 0.35
    got = check(ctx, f, 12, 3, True)
    for r in [0, 239] + [8 * k - 1 for k in range(1, 30)] + [8 * k for k in range(1, 30)]:
        on = f[r] != 0
        assert (got[r][on] == 0).any() and (got[r][on] == f[r][on]).any()
        assert ((got[r] != 0) & (got[r] != f[r])).any(), r
    check(ctx, f, 12, 3, False)
    check(ctx, f, 5, 1, True)
    assert np.array_equal(check(ctx, f, 0, 0, False), f)  # the identity


VIEWS = {"step 2": (640, 480, 640, 0, 0, 2, 0), "flip": (640, 480, 672, 0, 0, 2, 1),
         "pitch above width": (848, 480, 896, 0, 104, 2, 0),
         "step 3 odd origin": (1024, 1024, 1024, 151, 31, 3, 0),
         "negative origin": (640, 480, 640, -200, -300, 2, 0),
         "past the edges": (301, 241, 325, 0, 0, 2, 0),
         "outside": (640, 480, 640, 480, 0, 2, 0)}


@pytest.mark.parametrize("vname", sorted(VIEWS))
def test_through_a_view(ctx, vname):
    from hpe.view import View
    v = View(*VIEWS[vname])
    rng = np.random.default_rng(21)
    model = rng.integers(400, 460, size=(H, W)).astype(np.uint16)
    model[rng.random((H, W)) < 0.3] = 0
    cam = embed(v, model, 4)
    inside = v.camera_index()[2]
    red = v.reduce(cam)
    want = model[:, ::-1] if v.flip else model
    assert np.array_equal(red, np.where(inside, want, 0))  # the inputs are what the case needs
    assert (cam != 0).sum() > (red != 0).sum() and (cam[:, v.width:] != 0).all()
    if vname in ("negative origin", "past the edges"):
        assert 0 < inside.sum() < inside.size
    if vname == "outside":
        assert not inside.any()
    for edge, support, median in ((12, 3, True), (12, 2, False), (0, 0, False)):
        got = check(ctx, cam, edge, support, median, v)
        assert not got[~inside].any()
        assert got.any() == (vname != "outside")


def test_refusals(ctx):
    from hpe import _lib
    lib, h = ctx.lib, ctx.h
    f = np.full((H, W), 500, np.uint16)
    out = np.full((H, W), 7, np.uint16)
    fp, op = C.c_void_p(f.ctypes.data), C.c_void_p(out.ctypes.data)
    good = _lib.CleanPar(15, 3, 1, 0)
    E = _lib.HPE_E_ARG
    assert lib.hpe_clean_depth_u16(h, None, None, C.byref(good), op) == E
    assert lib.hpe_clean_depth_u16(h, fp, None, None, op) == E
    assert lib.hpe_clean_depth_u16(h, fp, None, C.byref(good), None) == E
    for bad in (_lib.CleanPar(15, 9, 0, 0), _lib.CleanPar(15, 3, 2, 0), _lib.CleanPar(15, 3, 0x81, 0),
                _lib.CleanPar(15, 3, 1, 1)):
        assert lib.hpe_clean_depth_u16(h, fp, None, C.byref(bad), op) == E
        assert lib.hpe_set_batch_clean(h, 1, C.byref(bad)) == E
    for bad_view in (_lib.View(640, 480, 640, 0, 0, 0, 0, 0), _lib.View(640, 480, 639, 0, 0, 2, 0, 0),
                     _lib.View(640, 480, 640, 0, 0, 2, 2, 0), _lib.View(640, 480, 640, 0, 0, 2, 0, 1)):
        assert lib.hpe_clean_depth_u16(h, fp, C.byref(bad_view), C.byref(good), op) == E
    assert (out == 7).all()  # nothing was written
    assert lib.hpe_set_batch_clean(h, 0, C.byref(good)) == E
    assert lib.hpe_set_batch_clean(h, 17, C.byref(good)) == E
    # no cleaned batch has begun on this context
    assert lib.hpe_batch_clean_readback(h, 0, 0, op) == _lib.HPE_E_STATE
    assert lib.hpe_batch_clean_readback(h, 0, 0, None) == E
    # the setting is off: turning it off again is accepted, and the context goes on
    assert lib.hpe_set_batch_clean(h, 0, None) == 0
    check(ctx, f, 15, 3, True)
