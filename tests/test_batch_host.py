"""CPU-side checks of the batched tracking call (hpe_track_batch_dev, no GPU):

* the entry point is exported and refuses a null context with HPE_E_ARG;
* Context.track_batch exists and checks its lane list on the Python side, before the
  library (and so without a device) is reached.
"""
import pytest


@pytest.fixture(scope="module")
def lib():
    from hpe import _lib
    return _lib.load()


def _no_device_context():
    """A Context that never reached hpe_create: only Python-side checks can run on it."""
    import hpe
    return object.__new__(hpe.Context)


def test_null_context_is_an_argument_error(lib):
    from hpe import _lib
    assert lib.hpe_track_batch_dev(None, 64, 1, 1, None, None, 1, 0, None) == _lib.HPE_E_ARG


def test_batch_max_matches_header():
    import re
    import hand_data
    from hpe import _lib
    txt = (hand_data.ROOT / "include" / "hpe.h").read_text()
    assert int(re.search(r"#define\s+HPE_BATCH_MAX\s+(\d+)", txt).group(1)) == _lib.BATCH_MAX == 16


def test_track_batch_rejects_an_empty_lane_list():
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.track_batch(64, 1, 0x1000, [], 1)


def test_track_batch_rejects_too_many_lanes():
    from hpe import _lib
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.track_batch(64, 1, 0x1000, [0] * (_lib.BATCH_MAX + 1), 1)


def test_track_batch_rejects_null_states():
    ctx = _no_device_context()
    with pytest.raises(ValueError):
        ctx.track_batch(64, 1, 0, [0, 1], 1)
