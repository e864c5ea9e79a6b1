"""CPU-side checks of the batched raw tracking call (hpe_track_raw_batch_dev, no GPU):

* the entry point is declared in include/hpe.h, exported by libhpe.so and present in the
  binding's signature table with its 12 arguments;
* it refuses a null context with HPE_E_ARG;
* Context.track_raw_batch checks its lane list on the Python side, before the library (and so
  without a device) is reached.
"""
import re
import subprocess

import pytest

import hand_data

NAME = "hpe_track_raw_batch_dev"
PKG = hand_data.ROOT / "hand-pose-estimation_amd"


def _no_device_context():
    """A Context that never reached hpe_create: only Python-side checks can run on it."""
    import hpe
    return object.__new__(hpe.Context)


def test_declared_in_the_header():
    txt = (hand_data.ROOT / "include" / "hpe.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", txt)
    assert m, "no declaration"
    assert len(m.group(1).split(",")) == 12


def test_exported_by_the_library():
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libhpe.so")],
                        capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + NAME + r"$", nm, flags=re.M)


def test_in_the_signature_table_with_12_arguments():
    from hpe import _lib
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == 12
    lib = _lib.load()
    assert getattr(lib, NAME).argtypes == args
    assert getattr(lib, NAME)(None, 64, 1, 1, None, None, 1, 1, 1, 241.42, 0, None) == _lib.HPE_E_ARG


@pytest.mark.parametrize("lanes", [0, 17])
def test_track_raw_batch_rejects_the_lane_count(lanes):
    from hpe import _lib
    assert _lib.BATCH_MAX == 16
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.track_raw_batch(64, 1, 0x1000, [0x2000] * lanes, 1)


def test_track_raw_batch_rejects_null_states():
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.track_raw_batch(64, 1, 0, [0x2000, 0x2000], 1)
