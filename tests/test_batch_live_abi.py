"""CPU-side checks of the live batch calls (hpe_batch_pipeline_begin, hpe_track_batch_pipelined;
no GPU):

* both entry points are declared in include/hpe.h with 6 arguments each, exported by libhpe.so
  and present in the binding's signature table;
* both refuse a null context with HPE_E_ARG;
* Context.batch_pipeline_begin and Context.track_batch_pipelined check the lane count, the states
  pointer and a partly-None frame list on the Python side, before the library (and so without a
  device) is reached.
"""
import re
import subprocess

import numpy as np
import pytest

import hand_data

NAMES = ("hpe_batch_pipeline_begin", "hpe_track_batch_pipelined")
PKG = hand_data.ROOT / "hand-pose-estimation_amd"
FRAME = np.zeros((240, 320), dtype=np.float32)


def _no_device_context():
    """A Context that never reached hpe_create: only Python-side checks can run on it."""
    import hpe
    return object.__new__(hpe.Context)


@pytest.mark.parametrize("name", NAMES)
def test_declared_in_the_header_with_6_arguments(name):
    txt = (hand_data.ROOT / "include" / "hpe.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert m, "no declaration"
    assert len(m.group(1).split(",")) == 6
    assert re.search(r"#define\s+HPE_ABI_VERSION\s+1\b", txt)


@pytest.mark.parametrize("name", NAMES)
def test_exported_by_the_library(name):
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libhpe.so")],
                        capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + name + r"$", nm, flags=re.M)


def test_in_the_signature_table_and_null_context_is_refused():
    from hpe import _lib
    lib = _lib.load()
    for name in NAMES:
        res, args = _lib.SIGNATURES[name]
        assert len(args) == 6
        assert getattr(lib, name).argtypes == args
    assert lib.hpe_batch_pipeline_begin(None, 1, None, 1, 1, 241.42) == _lib.HPE_E_ARG
    assert lib.hpe_track_batch_pipelined(None, 64, 1, 1, None, None) == _lib.HPE_E_ARG


@pytest.mark.parametrize("lanes", [0, 17])
def test_the_lane_count_is_checked_in_python(lanes):
    from hpe import _lib
    assert _lib.BATCH_MAX == 16
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.batch_pipeline_begin([FRAME] * lanes)
    with pytest.raises(ValueError):
        ctx.track_batch_pipelined(64, 1, 0x1000, [FRAME] * lanes)


def test_null_states_are_refused_in_python():
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.track_batch_pipelined(64, 1, 0, [FRAME, FRAME])
    with pytest.raises(ValueError):
        ctx.track_batch_pipelined(64, 1, 0, None)


def test_a_partly_none_frame_list_is_refused_in_python():
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.batch_pipeline_begin([FRAME, None])
    with pytest.raises(ValueError):
        ctx.track_batch_pipelined(64, 1, 0x1000, [None, FRAME, FRAME])
