"""CPU-side checks of the batch form calls (hpe_set_batch_form, hpe_batch_wave_wpp; no GPU):

* both entry points are declared in include/hpe.h (2 and 3 arguments), exported by libhpe.so and
  present in the binding's signature table;
* HPE_BATCH_FORM_AUTO is 0 and HPE_BATCH_FORM_WAVE is 1 in the header, and the binding mirrors
  them;
* both refuse a null context with HPE_E_ARG;
* Context.set_batch_form refuses an unknown form name on the Python side, before the library (and
  so without a device) is reached.
"""
import re
import subprocess

import pytest

import hand_data

NAMES = {"hpe_set_batch_form": 2, "hpe_batch_wave_wpp": 3}
PKG = hand_data.ROOT / "hand-pose-estimation_amd"


def _header():
    return (hand_data.ROOT / "include" / "hpe.h").read_text()


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_in_the_header(name):
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert m, "no declaration"
    assert len(m.group(1).split(",")) == NAMES[name]
    assert re.search(r"#define\s+HPE_ABI_VERSION\s+1\b", txt)


def test_the_form_constants():
    from hpe import _lib
    import hpe
    txt = _header()
    assert re.search(r"#define\s+HPE_BATCH_FORM_AUTO\s+0\b", txt)
    assert re.search(r"#define\s+HPE_BATCH_FORM_WAVE\s+1\b", txt)
    assert (_lib.BATCH_FORM_AUTO, _lib.BATCH_FORM_WAVE) == (0, 1)
    assert hpe.BATCH_FORMS == {"auto": 0, "wave": 1}


def test_the_header_states_form_wpp_rule_and_yardstick():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+HPE_BATCH_FORM_AUTO", _header(), flags=re.S)
    assert m, "no comment above the form constants"
    text = " ".join(m.group(1).split())
    for needle in ("HPE_BATCH_FORM_WAVE", "HPE_PSO_WPP", "B * num_p <= 1024", "HPE_PSO_FORM=wave",
                   "HPE_E_STATE", "hpe_track_raw_batch_dev", "hpe_track_batch_pipelined"):
        assert needle in text, needle


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
    for form in (_lib.BATCH_FORM_AUTO, _lib.BATCH_FORM_WAVE, 2, -1):
        assert lib.hpe_set_batch_form(None, form) == _lib.HPE_E_ARG
    assert lib.hpe_batch_wave_wpp(None, 64, 3) == _lib.HPE_E_ARG


def test_an_unknown_form_name_is_refused_in_python():
    import hpe
    ctx = object.__new__(hpe.Context)  # never reached hpe_create
    with pytest.raises(ValueError):
        ctx.set_batch_form("block")
