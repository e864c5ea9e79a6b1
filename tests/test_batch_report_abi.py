"""CPU-side checks of the lane reports (hpe_set_batch_report and its read calls,
hpe_lane_joints_dev; no GPU):

* the entry points are declared in include/hpe.h, exported by libhpe.so and in the binding's
  signature table with matching argument types; a null context is refused with HPE_E_ARG;
* hpe_lane_report_size() is ctypes.sizeof(LaneReport), 1096, and the binding's field offsets are
  the header's (computed from the header's own field list, every field naturally aligned);
* hpe.report.project_joints has known answers: the principal point for a joint on the optical
  axis, NaN for z <= 0 and for a non-finite coordinate, fp64 with each product rounded first;
* the ring reader (csrc/hpe_report.hpp) against a writer thread that plays the kernel's
  publication order: tests/cpp/report_ring_host.cpp, a stand-alone host program -- the newest
  report, the overwritten slot, and never a half-written one.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import hand_data

NAMES = {"hpe_lane_report_size": 1, "hpe_set_batch_report": 3, "hpe_batch_report": 4,
         "hpe_batch_report_wait": 5, "hpe_batch_lost": 2, "hpe_lane_joints_dev": 7}
PKG = hand_data.ROOT / "hand-pose-estimation_amd"


def _header():
    txt = (hand_data.ROOT / "include" / "hpe.h").read_text()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_exported_and_in_the_signature_table(name):
    from hpe import _lib
    m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, "no declaration"
    assert len(m.group(2).split(",")) == NAMES[name]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libhpe.so")],
                        capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + name + r"$", nm, flags=re.M)
    res, args = _lib.SIGNATURES[name]
    if name == "hpe_lane_report_size":
        assert m.group(1) == "size_t" and m.group(2).strip() == "void"
        assert res is C.c_size_t and args == []
    else:
        assert res is C.c_int and len(args) == NAMES[name]
    assert getattr(_lib.load(), name).argtypes == args


def test_argument_types_match_the_header():
    from hpe import _lib
    txt = _header()
    S = _lib.SIGNATURES
    assert re.search(r"int\s+hpe_set_batch_report\s*\(\s*hpe_ctx\s*\*\s*ctx\s*,\s*int\s+depth\s*,\s*"
                     r"const\s+hpe_report_watch\s*\*\s*watch\s*\)\s*;", txt)
    assert S["hpe_set_batch_report"][1] == [C.c_void_p, C.c_int, C.POINTER(_lib.ReportWatch)]
    assert re.search(r"int\s+hpe_batch_report\s*\(\s*hpe_ctx\s*\*\s*ctx\s*,\s*int\s+lane\s*,\s*"
                     r"uint64_t\s+seq\s*,\s*hpe_lane_report\s*\*\s*out\s*\)\s*;", txt)
    assert S["hpe_batch_report"][1] == [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(_lib.LaneReport)]
    assert re.search(r"int\s+hpe_batch_report_wait\s*\(\s*hpe_ctx\s*\*\s*ctx\s*,\s*int\s+lane\s*,\s*"
                     r"uint64_t\s+seq\s*,\s*int\s+timeout_ms\s*,\s*hpe_lane_report\s*\*\s*out\s*\)\s*;", txt)
    assert S["hpe_batch_report_wait"][1] == [C.c_void_p, C.c_int, C.c_uint64, C.c_int,
                                             C.POINTER(_lib.LaneReport)]
    assert re.search(r"int\s+hpe_batch_lost\s*\(\s*hpe_ctx\s*\*\s*ctx\s*,\s*uint32_t\s*\*\s*mask_out\s*\)\s*;", txt)
    assert S["hpe_batch_lost"][1] == [C.c_void_p, C.POINTER(C.c_uint32)]
    assert re.search(r"int\s+hpe_lane_joints_dev\s*\(\s*hpe_ctx\s*\*\s*ctx\s*,\s*int\s+B\s*,\s*int\s+n\s*,\s*"
                     r"const\s+double\s*\*\s*d_hist\s*,\s*double\s+focal\s*,\s*double\s*\*\s*d_joints\s*,"
                     r"\s*double\s*\*\s*d_px\s*\)\s*;", txt)
    assert S["hpe_lane_joints_dev"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                           C.c_void_p, C.c_void_p]
    # the constants
    for name, val in (("HPE_REPORT_TRACK", _lib.REPORT_TRACK), ("HPE_REPORT_INIT", _lib.REPORT_INIT),
                      ("HPE_REPORT_F_NAN", _lib.REPORT_F_NAN), ("HPE_REPORT_F_EMPTY", _lib.REPORT_F_EMPTY),
                      ("HPE_REPORT_F_SUSPECT", _lib.REPORT_F_SUSPECT),
                      ("HPE_REPORT_F_LOST", _lib.REPORT_F_LOST)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", txt)
        assert m and int(m.group(1)) == val, name
    assert (_lib.REPORT_TRACK, _lib.REPORT_INIT) == (1, 2)
    assert (_lib.REPORT_F_NAN, _lib.REPORT_F_EMPTY, _lib.REPORT_F_SUSPECT, _lib.REPORT_F_LOST) == (1, 2, 4, 8)


CTYPE_SIZE = {"uint64_t": 8, "int32_t": 4, "double": 8}


def _header_fields(struct_name):
    """[(field, offset, bytes)] of a typedef'd struct of the header, laid out by natural
    alignment, and the struct's size."""
    m = re.search(r"typedef\s+struct\s*(?:\w+\s*)?\{([^}]*)\}\s*" + struct_name + r"\s*;", _header())
    assert m, struct_name
    out, at, align = [], 0, 1
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        ty, rest = decl.split(None, 1)
        sz = CTYPE_SIZE[ty]
        align = max(align, sz)
        for f in (x.strip() for x in rest.split(",")):
            dims = [int(d) for d in re.findall(r"\[(\d+)\]", f)]
            name = re.match(r"\w+", f).group(0)
            at = (at + sz - 1) // sz * sz
            nbytes = sz * int(np.prod(dims)) if dims else sz
            out.append((name, at, nbytes))
            at += nbytes
    return out, (at + align - 1) // align * align


def test_lane_report_layout():
    from hpe import _lib
    fields, size = _header_fields("hpe_lane_report")
    assert size == 1096
    assert C.sizeof(_lib.LaneReport) == 1096
    assert _lib.load().hpe_lane_report_size() == 1096
    assert [f for f, _, _ in fields] == [f for f, _ in _lib.LaneReport._fields_]
    for name, off, nbytes in fields:
        d = getattr(_lib.LaneReport, name)
        assert (d.offset, d.size) == (off, nbytes), name
    assert {n: o for n, o, _ in fields} == {
        "seq": 0, "call": 8, "lane": 16, "kind": 20, "n": 24, "flags": 28, "bad_streak": 32,
        "pad": 36, "state": 40, "joints": 256, "px": 760}
    wf, wsize = _header_fields("hpe_report_watch")
    assert wsize == C.sizeof(_lib.ReportWatch) == 16
    for name, off, nbytes in wf:
        d = getattr(_lib.ReportWatch, name)
        assert (d.offset, d.size) == (off, nbytes), name


def test_null_context_is_refused():
    from hpe import _lib
    lib = _lib.load()
    r = _lib.LaneReport()
    m = C.c_uint32(0)
    assert lib.hpe_set_batch_report(None, 4, None) == _lib.HPE_E_ARG
    assert lib.hpe_batch_report(None, 0, 0, C.byref(r)) == _lib.HPE_E_ARG
    assert lib.hpe_batch_report_wait(None, 0, 0, 1, C.byref(r)) == _lib.HPE_E_ARG
    assert lib.hpe_batch_lost(None, C.byref(m)) == _lib.HPE_E_ARG
    assert lib.hpe_lane_joints_dev(None, 1, 1, None, 241.42, None, None) == _lib.HPE_E_ARG


def test_python_side_argument_checks():
    import hpe
    ctx = object.__new__(hpe.Context)  # never reached hpe_create
    with pytest.raises((TypeError, ValueError)):
        ctx.set_batch_report(4, watch=(1.0, 2))  # a watch is (cost_max, n_min, streak)
    with pytest.raises(ValueError):
        hpe.report.project_joints(np.zeros((21, 2)))


# ---- the pixel rule's host mirror
def test_project_joints_known_answers():
    from hpe.report import project_joints
    f = 241.42
    # on the optical axis: the principal point, whatever the depth
    for z in (1.0, 32.0, 1e-3, 1e6):
        assert np.array_equal(project_joints([[0.0, 0.0, z]], f), [[160.0, 120.0]])
    # one focal length per unit of x / z and y / z (powers of two: every operation exact)
    assert np.array_equal(project_joints([[2.0, -4.0, 8.0]], 256.0), [[160.0 + 64.0, 120.0 - 128.0]])
    # behind or at the camera, and non-finite coordinates: both NaN
    bad = [[1.0, 2.0, 0.0], [1.0, 2.0, -5.0], [np.nan, 2.0, 30.0], [1.0, np.inf, 30.0],
           [1.0, 2.0, np.inf], [1.0, 2.0, np.nan], [-np.inf, 0.0, 30.0]]
    out = project_joints(bad, f)
    assert out.shape == (7, 2) and np.isnan(out).all()
    # a bad joint leaves its neighbours alone; shapes carry through
    j = np.zeros((2, 21, 3))
    j[..., 2] = 30.0
    j[1, 7] = (1.0, 1.0, -1.0)
    out = project_joints(j, f)
    assert out.shape == (2, 21, 2) and out.dtype == np.float64
    assert np.isnan(out[1, 7]).all() and np.isfinite(np.delete(out.reshape(42, 2), 28, axis=0)).all()


def test_project_joints_rounds_each_product_before_its_add():
    """(focal x + 160 z) / z with the two products and the sum rounded one by one: checked
    against the same steps in exact rational arithmetic, rounded to fp64 after each."""
    from fractions import Fraction

    from hpe.report import project_joints
    rng = np.random.default_rng(7)
    J = np.column_stack([rng.uniform(-20, 20, 64), rng.uniform(-20, 20, 64), rng.uniform(15, 60, 64)])
    f = 241.42
    got = project_joints(J, f)

    def rnd(q):
        return Fraction(float(q))  # float(Fraction) rounds to nearest even

    for (x, y, z), (col, row) in zip(J, got):
        for v, c, g in ((x, 160.0, col), (y, 120.0, row)):
            num = rnd(rnd(Fraction(f) * Fraction(v)) + rnd(Fraction(c) * Fraction(z)))
            assert float(num / Fraction(z)) == g


# ---- the ring reader against a writer thread
def _build_ring_test(d):
    exe = d / "report_ring_host"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-o", str(exe),
                    str(hand_data.ROOT / "tests" / "cpp" / "report_ring_host.cpp"),
                    f"-I{PKG / 'csrc'}"], check=True, timeout=120)
    return exe


def test_ring_reader_against_a_writer_thread(tmp_path):
    exe = _build_ring_test(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "report ring: ok" in out.stdout
