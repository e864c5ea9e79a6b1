"""CPU-side checks of lane location (hpe_locate_defaults, hpe_locate_depth,
hpe_batch_pipeline_locate, hpe_batch_locate_result; no GPU):

* hpe_locate_params and hpe_locate: the binding's sizes and field offsets are the C compiler's on
  include/hpe.h; the defaults of the library, of the header's text and of the mirror agree; null
  pointers are refused with HPE_E_ARG;
* known answers of the numpy mirror hpe/locate.py, worked out by hand from the rule;
* the scene condition: on a rendered hand in front of a wall, with a forearm and speckle, the
  located window keeps every rendered hand pixel and no wall pixel, at the defaults;
* the placement rule: the placed row's sphere centroid lands on the centre (1e-9 cm, the project's
  FK tolerance), under the numpy hand model.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hand_data
import oracle_np

FOCAL = 241.42
HEADER = hand_data.ROOT / "include"


def test_struct_layouts_match_the_compiler(tmp_path):
    from hpe import _lib
    fields = {"hpe_locate_params": [f for f, _ in _lib.LocateParams._fields_],
              "hpe_locate": [f for f, _ in _lib.Locate._fields_]}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "hpe.h"', "int main(void) {"]
    for s, fs in fields.items():
        src.append(f'printf("{s} %zu\\n", sizeof({s}));')
        src += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    src += ["return 0; }"]
    (tmp_path / "lay.c").write_text("\n".join(src))
    exe = tmp_path / "lay"
    subprocess.run(["cc", "-std=c11", f"-I{HEADER}", "-o", str(exe), str(tmp_path / "lay.c")],
                   check=True, timeout=60)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                   check=True, timeout=60).stdout.splitlines())
    for s, cls in (("hpe_locate_params", _lib.LocateParams), ("hpe_locate", _lib.Locate)):
        assert int(got[s]) == C.sizeof(cls)
        for f in fields[s]:
            assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, (s, f)
    assert C.sizeof(_lib.LocateParams) == 72 and C.sizeof(_lib.Locate) == 104


def test_defaults_and_null_pointers():
    from hpe import _lib, locate
    lib = _lib.load()
    p = _lib.LocateParams()
    assert lib.hpe_locate_defaults(C.byref(p)) == 0
    got = locate.Params(tuple(getattr(p.search, f) for f, _ in _lib.Window._fields_), p.bin, p.slab,
                        p.half_xy, p.half_z, p.skip, p.min_pixels)
    assert got == locate.Params(tuple(locate.DEFAULTS.search), 0.5, 12.0, 11.0, 11.0, 20, 200)
    assert locate.as_params(got) == locate.DEFAULTS
    assert lib.hpe_locate_defaults(None) == _lib.HPE_E_ARG
    r = _lib.Locate()
    frame = np.zeros((240, 320), np.float32)
    assert lib.hpe_locate_depth(None, frame.ctypes.data, 0, 1.0, 1, FOCAL, None, C.byref(r)) == _lib.HPE_E_ARG
    assert lib.hpe_batch_pipeline_locate(None, 1, None, 1, None, None) == _lib.HPE_E_ARG
    assert lib.hpe_batch_locate_result(None, 0, 0, C.byref(r)) == _lib.HPE_E_ARG


def rect(rows, cols, mm, base=None):
    d = np.zeros((240, 320), np.float32) if base is None else base.copy()
    d[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = mm
    return d


def test_mirror_empty_frame():
    from hpe import locate
    r = locate.locate(np.zeros((240, 320), np.float32), FOCAL)
    assert r == locate.Result(0, -1, 0, 0, (0.0, 0.0), (0.0, 0.0, 0.0), locate.NO_WINDOW)


def test_mirror_one_rectangle():
    """Rows 100..139, columns 150..199 at 400 mm = 40 cm: bin 80 of 0.5 cm, z = 80.5 * 0.5."""
    from hpe import locate, window
    r = locate.locate(rect((100, 139), (150, 199), 400.0), FOCAL)
    z = 40.25
    hx = (FOCAL * 11.0) / z
    assert (r.found, r.k_near, r.m1, r.m2) == (1, 80, 2000, 2000)
    assert r.px == (174.5, 119.5)
    assert r.centre == (((174.5 - 160.0) * z) / FOCAL, ((119.5 - 120.0) * z) / FOCAL, z)
    assert r.window == window.Window(int(np.ceil(119.5 - hx)), int(np.floor(119.5 + hx)),
                                     int(np.ceil(174.5 - hx)), int(np.floor(174.5 + hx)),
                                     z - 11.0, z + 11.0)
    assert r.window == window.Window(54, 185, 109, 240, 29.25, 51.25)


def test_mirror_speckle_and_skip():
    """`skip` speckle pixels nearer than the object do not move k_near; one more does."""
    from hpe import locate
    d = rect((100, 139), (150, 199), 400.0)
    clean = locate.locate(d, FOCAL)
    sp = d.copy()
    sp[5, 10:30] = 150.0  # 20 pixels at 15 cm: bin 30
    assert locate.DEFAULTS.skip == 20
    r = locate.locate(sp, FOCAL)
    assert r.k_near == 80 and r.m1 == 2000 and r.centre == clean.centre and r.window == clean.window
    sp[5, 30] = 150.0     # the 21st
    r = locate.locate(sp, FOCAL)
    assert r.k_near == 30 and r.m1 == 21  # the slab 15 .. 27.5 cm holds the speckle alone
    assert locate.locate(sp, FOCAL, locate.DEFAULTS._replace(skip=21)).k_near == 80
    assert locate.locate(sp, FOCAL, locate.DEFAULTS._replace(skip=0)).k_near == 30


def test_mirror_search_excludes_a_nearer_object():
    from hpe import locate, window
    d = rect((100, 139), (150, 199), 400.0)
    clean = locate.locate(d, FOCAL)
    d2 = rect((0, 239), (0, 40), 200.0, base=d)  # a nearer object on the left
    assert locate.locate(d2, FOCAL).k_near == 40
    p = locate.DEFAULTS._replace(search=window.Window(0, 239, 100, 319, -np.inf, np.inf))
    r = locate.locate(d2, FOCAL, p)
    assert (r.k_near, r.m1, r.m2, r.px, r.centre) == (80, 2000, 2000, clean.px, clean.centre)
    # the box is clamped to the search window
    assert r.window == clean.window._replace(col_lo=max(clean.window.col_lo, 100))
    # ... and by depth: the search range ends in front of the nearer object's bin
    p = locate.DEFAULTS._replace(search=window.Window(0, 239, 0, 319, 30.0, 45.0))
    r = locate.locate(d2, FOCAL, p)
    assert (r.k_near, r.m1) == (80, 2000) and (r.window.z_lo, r.window.z_hi) == (30.0, 45.0)


def test_mirror_box_clipped_by_the_image_edge():
    from hpe import locate
    r = locate.locate(rect((0, 29), (290, 319), 400.0), FOCAL, locate.DEFAULTS._replace(min_pixels=1))
    assert r.found == 1 and r.px == (304.5, 14.5)
    assert (r.window.row_lo, r.window.col_hi) == (0, 319)
    assert (r.window.row_hi, r.window.col_lo) == (80, 239)  # 14.5 + 65.98.., 304.5 - 65.98..


def test_mirror_too_few_pixels():
    from hpe import locate
    d = rect((100, 109), (150, 159), 400.0)  # 100 pixels < min_pixels = 200
    r = locate.locate(d, FOCAL)
    assert r == locate.Result(0, 80, 100, 100, (0.0, 0.0), (0.0, 0.0, 0.0), locate.NO_WINDOW)
    assert locate.locate(d, FOCAL, locate.DEFAULTS._replace(min_pixels=100)).found == 1


def test_mirror_u16_and_raw_unit():
    """A u16 frame is the float frame float32(u) * float32(unit); to_cm = 0 reads Z in mm."""
    from hpe import locate
    u = np.zeros((240, 320), np.uint16)
    u[100:140, 150:200] = 40000  # above 32767
    unit = np.float32(0.01)
    a = locate.locate(u, FOCAL, unit_mm=unit)
    b = locate.locate(u.astype(np.float32) * unit, FOCAL)
    assert a == b and a.found == 1 and a.k_near == 80
    mm = locate.DEFAULTS._replace(bin=5.0, slab=120.0, half_xy=110.0, half_z=110.0)
    c = locate.locate(u, FOCAL, mm, to_cm=False, unit_mm=unit)
    assert c.k_near == 80 and c.centre[2] == 402.5
    with pytest.raises(TypeError):
        locate.locate(u, FOCAL)


@pytest.mark.parametrize("frame", ["x0", 0, 4, 8])
def test_scene_window_keeps_the_hand_and_no_wall(np_hand, frame):
    """A rendered hand, a wall at 800 mm, a forearm from the wrist to the bottom edge 1 cm behind
    the wrist and 15 speckle pixels at 150 mm: at the defaults the located window keeps every
    rendered hand pixel and no wall pixel."""
    import hpe
    from hpe import locate, synth, window
    th = hpe.X0 if frame == "x0" else synth.trajectory(25)[frame]
    hand = oracle_np.render_depth_mm(np_hand, th)
    scene = synth.rig_scene(hand, th[3:6], FOCAL)
    assert (scene == 800.0).sum() > 30000 and (scene == 150.0).sum() == 15
    r = locate.locate(scene, FOCAL)
    assert r.found == 1
    keep = window.keep_mask(scene, r.window)
    on = hand > 0
    assert on.sum() > 5000
    assert (keep & on).sum() == on.sum()
    assert (keep & (scene == 800.0)).sum() == 0
    assert (keep & (scene == 150.0)).sum() == 0


def test_placement_puts_the_centroid_on_the_centre(np_hand):
    import hpe
    from hpe import locate
    T = np.asarray(hpe.X0, dtype=np.float64)
    S = locate.camera_centres(np_hand.build_hand_model(T))
    for centre in ((2.5, -1.0, 40.25), (-12.0, 7.0, 27.0)):
        row = locate.place(S, T, centre)
        assert np.array_equal(np.delete(row, [3, 4, 5]), np.delete(T, [3, 4, 5]))
        S2 = locate.camera_centres(np_hand.build_hand_model(row))
        assert np.abs(locate.centroid(S2) - np.array(centre)).max() <= 1e-9
