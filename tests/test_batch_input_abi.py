"""CPU-side checks of the live batch's lane input (hpe_batch_pipeline_begin_u16,
hpe_track_batch_pipelined_u16, hpe_batch_frame_buffer; no GPU):

* the entry points are declared in include/hpe.h, exported by libhpe.so and in the binding's
  signature table with the header's argument types; a null context is refused with HPE_E_ARG;
* hpe.depth_u16_to_mm, the host side of the conversion rule rv = (float)u * unit_mm, has known
  answers: the single-rounded fp32 product, float32 out, uint16 in and nothing else;
* Context.batch_pipeline_begin(input="u16") refuses float arrays in Python, before any library
  call (a stub context that never reached hpe_create).
"""
import ctypes as C
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hand_data

NAMES = {"hpe_batch_pipeline_begin_u16": 7, "hpe_track_batch_pipelined_u16": 6,
         "hpe_batch_frame_buffer": 4}
PKG = hand_data.ROOT / "hand-pose-estimation_amd"


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
    assert res is C.c_int and len(args) == NAMES[name]
    assert getattr(_lib.load(), name).argtypes == args


def test_argument_types_match_the_header():
    from hpe import _lib
    txt = _header()
    S = _lib.SIGNATURES
    assert re.search(r"int\s+hpe_batch_pipeline_begin_u16\s*\(\s*hpe_ctx\s*\*\s*ctx\s*,\s*int\s+B\s*,\s*"
                     r"const\s+uint16_t\s*\*\s*const\s*\*\s*depth\s*,\s*float\s+unit_mm\s*,\s*"
                     r"int\s+to_cm\s*,\s*int\s+downsample\s*,\s*double\s+focal\s*\)\s*;", txt)
    assert S["hpe_batch_pipeline_begin_u16"][1] == [C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                                    C.c_float, C.c_int, C.c_int, C.c_double]
    assert re.search(r"int\s+hpe_track_batch_pipelined_u16\s*\(\s*hpe_ctx\s*\*\s*ctx\s*,\s*int\s+num_p\s*,"
                     r"\s*int\s+refine\s*,\s*int\s+B\s*,\s*double\s*\*\s*d_states\s*,\s*"
                     r"const\s+uint16_t\s*\*\s*const\s*\*\s*next_depth\s*\)\s*;", txt)
    assert S["hpe_track_batch_pipelined_u16"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                     C.c_void_p, C.POINTER(C.c_void_p)]
    assert re.search(r"int\s+hpe_batch_frame_buffer\s*\(\s*hpe_ctx\s*\*\s*ctx\s*,\s*int\s+lane\s*,\s*"
                     r"void\s*\*\s*\*\s*buf_out\s*,\s*size_t\s*\*\s*bytes_out\s*\)\s*;", txt)
    assert S["hpe_batch_frame_buffer"][1] == [C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_size_t)]


def test_null_context_is_refused():
    from hpe import _lib
    lib = _lib.load()
    buf, n = C.c_void_p(), C.c_size_t(0)
    assert lib.hpe_batch_pipeline_begin_u16(None, 1, None, 1.0, 1, 1, 241.42) == _lib.HPE_E_ARG
    assert lib.hpe_track_batch_pipelined_u16(None, 64, 1, 1, None, None) == _lib.HPE_E_ARG
    assert lib.hpe_batch_frame_buffer(None, 0, C.byref(buf), C.byref(n)) == _lib.HPE_E_ARG


def _fp32_product(u, unit):
    """float32(u) * float32(unit) rounded once, by exact rational arithmetic: the float32 nearest
    the exact product (ties to even), found among the neighbours of the fp64 product -- exact
    itself, 16 + 24 significant bits."""
    exact = Fraction(int(u)) * Fraction(float(np.float32(unit)))
    near = np.float32(float(exact))
    cands = [np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - exact),
                                     int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


@pytest.mark.parametrize("unit", [1, 0.25, np.float32(0.0055)])
def test_depth_u16_to_mm_known_answers(unit):
    import hpe
    u = np.array([[0, 65535, 32768, 1, 40000]], dtype=np.uint16)
    got = hpe.depth_u16_to_mm(u, unit)
    assert got.dtype == np.float32 and got.shape == u.shape
    assert got[0, 0] == 0.0 and not np.signbit(got[0, 0])
    for k in range(u.shape[1]):
        want = _fp32_product(u[0, k], unit)
        assert got[0, k].view(np.uint32) == want.view(np.uint32), (u[0, k], unit)
    # values above 32767 are depths like the others: never negative
    assert (got[0, 1:] > 0).all()
    if unit == 1:
        assert got[0, 1] == 65535.0 and got[0, 2] == 32768.0
    if unit == 0.25:
        assert got[0, 1] == 16383.75 and got[0, 2] == 8192.0


def test_depth_u16_to_mm_takes_uint16_only():
    import hpe
    for bad in (np.zeros((2, 2), np.float32), np.zeros((2, 2), np.int16), np.zeros((2, 2), np.int32),
                [[1, 2]]):
        with pytest.raises(TypeError):
            hpe.depth_u16_to_mm(bad, 1.0)


def test_u16_begin_refuses_float_arrays_before_any_library_call():
    import hpe
    ctx = object.__new__(hpe.Context)  # never reached hpe_create: a library call would raise
    f32 = np.zeros((240, 320), np.float32)
    u16 = np.zeros((240, 320), np.uint16)
    with pytest.raises(TypeError):
        ctx.batch_pipeline_begin([f32], input="u16")
    with pytest.raises(TypeError):
        ctx.batch_pipeline_begin([u16, f32.astype(np.float64)], input="u16", unit_mm=0.25)
    with pytest.raises(TypeError):  # nor the other way round
        ctx.batch_pipeline_begin([u16])
    with pytest.raises(ValueError):
        ctx.batch_pipeline_begin([u16], input="u8")
    # the stub reaches the library only with well-formed frames
    with pytest.raises(AttributeError):
        ctx.batch_pipeline_begin([u16], input="u16")
