"""CPU-side checks of lane pacing (hpe_set_batch_pacing, hpe_batch_pending; no GPU):

* both entry points are declared in include/hpe.h, exported by libhpe.so and present in the
  binding's signature table; HPE_PACING_LOCKSTEP / HPE_PACING_FREE have their values;
* both refuse a null context with HPE_E_ARG;
* Context.set_batch_pacing refuses an unknown mode name in Python;
* Context.batch_pipeline_begin and Context.track_batch_pipelined pass a partly-None frame list on
  to the library (as null lane pointers) only after set_batch_pacing("free"); under the default
  they keep refusing it in Python.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import hand_data

NAMES = {"hpe_set_batch_pacing": 2, "hpe_batch_pending": 2}
PKG = hand_data.ROOT / "hand-pose-estimation_amd"
FRAME = np.zeros((240, 320), dtype=np.float32)


def _header():
    txt = (hand_data.ROOT / "include" / "hpe.h").read_text()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_in_the_header(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, "no declaration"
    assert len(m.group(1).split(",")) == NAMES[name]


def test_the_constants():
    from hpe import _lib
    txt = _header()
    assert re.search(r"#define\s+HPE_PACING_LOCKSTEP\s+0\b", txt)
    assert re.search(r"#define\s+HPE_PACING_FREE\s+1\b", txt)
    assert (_lib.PACING_LOCKSTEP, _lib.PACING_FREE) == (0, 1)


@pytest.mark.parametrize("name", sorted(NAMES))
def test_exported_by_the_library(name):
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libhpe.so")],
                        capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + name + r"$", nm, flags=re.M)


def test_in_the_signature_table_and_null_context_is_refused():
    from hpe import _lib
    lib = _lib.load()
    for name, nargs in NAMES.items():
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs
        assert getattr(lib, name).argtypes == args
    m = C.c_uint32(0xdead)
    assert lib.hpe_set_batch_pacing(None, 1) == _lib.HPE_E_ARG
    assert lib.hpe_batch_pending(None, C.byref(m)) == _lib.HPE_E_ARG
    assert m.value == 0xdead


class _RecordingLib:
    """Stands in for libhpe.so behind a Context that never reached hpe_create: every entry point
    returns HPE_OK and records its arguments, so what the Python wrappers pass on is visible."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _no_device_context():
    import hpe
    ctx = object.__new__(hpe.Context)
    ctx.lib = _RecordingLib()
    ctx._h = None
    return ctx


def test_an_unknown_mode_name_is_refused_in_python():
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.set_batch_pacing("ragged")
    assert not ctx.lib.calls
    ctx.set_batch_pacing("lockstep")
    ctx.set_batch_pacing("free")
    assert [c for c in ctx.lib.calls] == [("hpe_set_batch_pacing", (None, 0)),
                                          ("hpe_set_batch_pacing", (None, 1))]


def test_a_partly_none_list_is_accepted_only_under_free():
    ctx = _no_device_context()
    for mode in (None, "lockstep"):
        if mode:
            ctx.set_batch_pacing(mode)
        with pytest.raises(ValueError):
            ctx.batch_pipeline_begin([FRAME, None])
        with pytest.raises(ValueError):
            ctx.track_batch_pipelined(64, 1, 0x1000, [None, FRAME, FRAME])
    assert all(name == "hpe_set_batch_pacing" for name, _ in ctx.lib.calls)
    ctx.set_batch_pacing("free")
    ctx.batch_pipeline_begin([FRAME, None])
    name, args = ctx.lib.calls[-1]
    assert name == "hpe_batch_pipeline_begin" and args[1] == 2
    assert args[2][0] == FRAME.ctypes.data and args[2][1] is None
    ctx.track_batch_pipelined(64, 1, 0x1000, [None, FRAME, None])
    name, args = ctx.lib.calls[-1]
    assert name == "hpe_track_batch_pipelined" and args[3] == 3
    assert [args[5][b] for b in range(3)] == [None, FRAME.ctypes.data, None]
    ctx.track_batch_pipelined(64, 1, 0x1000, [None, None])  # every entry None: still an array
    name, args = ctx.lib.calls[-1]
    assert args[3] == 2 and args[5] is not None and args[5][0] is None and args[5][1] is None
    # the lane count is still checked
    with pytest.raises(ValueError):
        ctx.batch_pipeline_begin([None] * 17)
    # back to lockstep: refused in Python again
    ctx.set_batch_pacing("lockstep")
    with pytest.raises(ValueError):
        ctx.batch_pipeline_begin([FRAME, None])
