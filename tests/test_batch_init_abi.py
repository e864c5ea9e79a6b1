"""CPU-side checks of lane initialisation (hpe_pso_optimise_batch, hpe_batch_pipeline_optimise;
no GPU):

* both entry points are declared in include/hpe.h with 6 parameters each, exported by libhpe.so
  and present in the binding's signature table;
* both refuse a null context with HPE_E_ARG;
* Context.pso_optimise_batch and Context.batch_pipeline_optimise pass their arguments on: the
  lane count from the slot list / the begin, the mask as given, or all lanes (lockstep) /
  batch_pending() (free pacing) for lanes=None.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import hand_data

NAMES = {"hpe_pso_optimise_batch": 6, "hpe_batch_pipeline_optimise": 6}
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
    slots = (C.c_int32 * 2)(0, 1)
    assert lib.hpe_pso_optimise_batch(None, 16, 2, C.c_void_p(0x1000), slots, None) == _lib.HPE_E_ARG
    assert lib.hpe_batch_pipeline_optimise(None, 16, 2, C.c_void_p(0x1000), 3, None) == _lib.HPE_E_ARG


class _RecordingLib:
    """Stands in for libhpe.so behind a Context that never reached hpe_create: every entry point
    returns HPE_OK and records its arguments, so what the Python wrappers pass on is visible.
    hpe_batch_pending answers with `pending`."""

    def __init__(self, pending=0):
        self.calls = []
        self.pending = pending

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name == "hpe_batch_pending":
                args[1]._obj.value = self.pending
            return 0
        return call


def _no_device_context(pending=0):
    import hpe
    ctx = object.__new__(hpe.Context)
    ctx.lib = _RecordingLib(pending)
    ctx._h = None
    return ctx


def test_the_slot_wrapper_passes_its_arguments_on():
    ctx = _no_device_context()
    ctx.pso_optimise_batch(32, 0x1000, [5, 2, 5])
    name, args = ctx.lib.calls[-1]
    assert name == "hpe_pso_optimise_batch"
    assert args[0] is None and args[1] == 32 and args[2] == 3 and args[3].value == 0x1000
    assert list(args[4]) == [5, 2, 5] and args[5] is None
    ctx.pso_optimise_batch(8, 0x1000, [7], d_trace_ptr=0x2000)
    name, args = ctx.lib.calls[-1]
    assert args[1] == 8 and args[2] == 1 and list(args[4]) == [7] and args[5].value == 0x2000
    n = len(ctx.lib.calls)
    with pytest.raises(ValueError):
        ctx.pso_optimise_batch(8, 0x1000, [])
    with pytest.raises(ValueError):
        ctx.pso_optimise_batch(8, 0x1000, [0] * 17)
    with pytest.raises(ValueError):
        ctx.pso_optimise_batch(8, 0, [0])
    assert len(ctx.lib.calls) == n


def test_the_live_wrapper_passes_its_arguments_on():
    ctx = _no_device_context()
    ctx.batch_pipeline_begin([FRAME, FRAME, FRAME])
    ctx.batch_pipeline_optimise(16, 0x1000)  # lockstep, lanes=None: every lane of the begin
    name, args = ctx.lib.calls[-1]
    assert name == "hpe_batch_pipeline_optimise"
    assert args[0] is None and args[1] == 16 and args[2] == 3 and args[3].value == 0x1000
    assert args[4] == 0b111 and args[5] is None
    ctx.batch_pipeline_optimise(16, 0x1000, lanes=0b010, d_trace_ptr=0x2000)
    name, args = ctx.lib.calls[-1]
    assert args[2] == 3 and args[4] == 0b010 and args[5].value == 0x2000
    with pytest.raises(ValueError):
        ctx.batch_pipeline_optimise(16, 0)


def test_the_live_wrapper_takes_the_pending_lanes_under_free_pacing():
    ctx = _no_device_context(pending=0b101)
    ctx.set_batch_pacing("free")
    ctx.batch_pipeline_begin([FRAME, None, FRAME])
    ctx.batch_pipeline_optimise(16, 0x1000)
    assert [n for n, _ in ctx.lib.calls[-2:]] == ["hpe_batch_pending", "hpe_batch_pipeline_optimise"]
    args = ctx.lib.calls[-1][1]
    assert args[2] == 3 and args[4] == 0b101
    ctx.batch_pipeline_optimise(16, 0x1000, lanes=0b001)  # an explicit mask asks nothing
    assert ctx.lib.calls[-2][0] == "hpe_batch_pipeline_optimise"
    assert ctx.lib.calls[-1][1][4] == 0b001
