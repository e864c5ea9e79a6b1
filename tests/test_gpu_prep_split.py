"""The distance transform split over two refine launches (hpe_track_raw_sequence_dev, DESIGN.md
§4.4): refine launch f scans frame f+1 backward from the forward values launch f-1 (or the call's
prologue) left, beside the forward scan of frame f+2 for launch f+1.

The yardstick is the per-frame hpe_track_pipelined loop, which keeps the whole transform in one
launch: histories and final states must be equal bit for bit (both scans are integer min-plus
arithmetic), for every sequence length and chunking that moves the hand-off -- both buffer
parities, chunks whose last frame has a next frame but no frame after it, a sequence's last two
frames -- and for frames at the scans' edges.  The prepared buffers themselves are read back
(hpe_pipe_readback) against the host preprocessing.  The chunk graphs must not depend on the
sequence length, and HPE_PREP_SPLIT=0 (read at hpe_create) must give the same bits.

Run as a script (the switch test's child process): FRAMES.npy OUT.npy P maxiter n K."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SEQ, P_SEQ, MAXITER = 7, 16, 4


def _set_params(ctx, maxiter):
    import hpe
    import oracle_np
    ub, lb, sd = oracle_np.reference_bounds()
    pso = hpe.PSO()
    pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, maxiter, 1e-8, 1e-8)
    pso._push(ctx)


def _state(x0):
    import torch
    st = torch.zeros(27, dtype=torch.float64, device="cuda:0")
    st[:26] = torch.from_numpy(x0)
    torch.cuda.synchronize()
    return st


def _pipelined(ctx, depth, P, refine=1, downsample=True):
    """The yardstick: one hpe_track_pipelined call per frame, {bestp, cost} after each."""
    import oracle_np
    st = _state(oracle_np.X0)
    ctx.pipeline_begin(depth[0], downsample=downsample)
    out = []
    for f in range(len(depth)):
        ctx.track_pipelined(P, refine, st.data_ptr(), depth[f + 1] if f + 1 < len(depth) else None)
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        out.append(st.cpu().numpy().copy())
    return np.array(out)


def _buffers():
    import torch
    return (torch.zeros(27, dtype=torch.float64, device="cuda:0"),
            torch.empty((N_SEQ, 27), dtype=torch.float64, device="cuda:0"))


def _raw_sequence(ctx, d_raw, n, P, K, bufs, refine=1, downsample=True):
    """hpe_track_raw_sequence_dev over the first n frames of d_raw; (history, final state).
    bufs: the device state and history (part of the chunk graphs' key)."""
    import oracle_np
    import torch
    st, hist = bufs
    st[:26] = torch.from_numpy(oracle_np.X0)
    st[26] = 0.0
    hist.fill_(float("nan"))
    torch.cuda.synchronize()
    ctx.track_raw_sequence(P, refine, st.data_ptr(), d_raw.data_ptr(), n, downsample=downsample,
                           frames_per_graph=K, d_hist_ptr=hist.data_ptr())
    ctx.check(ctx.lib.hpe_sync(ctx.h))
    return hist.cpu().numpy()[:n].copy(), st.cpu().numpy().copy()


def _to_dev(depth):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(depth), dtype=np.float32)).to("cuda:0")


def _check_buffer(got, want):
    np.testing.assert_array_equal(got["depth_cm"], want["depth_cm"])
    np.testing.assert_array_equal(got["dt"], want["dt"])
    np.testing.assert_array_equal(got["cloud"], want["cloud"])
    assert got["dtmax"] == want["dtmax"]
    assert got["scale"] == want["scale"] or (np.isnan(got["scale"]) and np.isnan(want["scale"]))


@pytest.fixture(scope="module")
def gh():
    import hpe
    return hpe.reference_hand(device=0)


@pytest.fixture(scope="module")
def depth(np_hand):
    import hand_data
    import oracle_np
    return [oracle_np.render_depth_mm(np_hand, th) for th in hand_data.trajectory(N_SEQ, seed=47)]


@pytest.fixture(scope="module")
def d_raw(depth):
    return _to_dev(depth)


@pytest.fixture(scope="module")
def bufs():
    return _buffers()


@pytest.fixture(scope="module")
def ref(gh, depth):
    """The pipelined loop over the module's frames, once; frame f's row does not depend on how
    many frames follow it, so a prefix of it is the yardstick of every shorter sequence."""
    _set_params(gh.ctx, MAXITER)
    return _pipelined(gh.ctx, depth, P_SEQ)


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_bit_identity_frame_by_frame(gh, d_raw, ref, bufs, n):
    _set_params(gh.ctx, MAXITER)
    for K in (0, 1, 2, 3, 8):
        hist, final = _raw_sequence(gh.ctx, d_raw, n, P_SEQ, K, bufs)
        assert np.array_equal(hist, ref[:n]), (n, K)
        assert np.array_equal(final, ref[n - 1]), (n, K)


def test_bit_identity_full_cloud_multi_workgroup_refine(gh, depth, bufs):
    """downsample off: ~9k-point clouds, the multi-workgroup refine (1 + 64 helpers + 9)."""
    _set_params(gh.ctx, 3)
    d3 = depth[:3]
    want = _pipelined(gh.ctx, d3, 8, downsample=False)
    hist, final = _raw_sequence(gh.ctx, _to_dev(d3), 3, 8, 2, bufs, downsample=False)
    assert np.array_equal(hist, want)
    assert np.array_equal(final, want[-1])


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_prepared_buffers(gh, depth, d_raw, bufs, m):
    """After m frames (refine off: the preparation rides in launches that refine nothing) buffer
    (m-1) & 1 holds frame m-1 and the other one frame m-2, as the host prepares them."""
    import hpe
    _set_params(gh.ctx, 3)
    _raw_sequence(gh.ctx, d_raw, m, 8, 0, bufs, refine=0)
    for f in (m - 1, m - 2):
        if f >= 0:
            _check_buffer(gh.ctx.pipe_readback(f & 1), hpe.preprocess_depth(depth[f]))


def _edge_frames(base):
    """Frames at the scans' edges, cut from a rendered hand frame."""
    rows = np.flatnonzero(base.any(axis=1))
    cols = np.flatnonzero(base.any(axis=0))
    zero = np.zeros_like(base)
    top = np.roll(base, -rows[0], axis=0)           # the hand's first row is row 0
    bottom = np.roll(base, 239 - rows[-1], axis=0)  # its last row is row 239
    left = np.roll(base, -cols[0], axis=1)
    right = np.roll(base, 319 - cols[-1], axis=1)
    sides = np.where(left != 0, left, right)        # hands touching columns 0 and 319
    assert top[0].any() and bottom[239].any() and sides[:, 0].any() and sides[:, 319].any()
    return {"zero": zero, "row0": top, "row239": bottom, "cols0_319": sides}


@pytest.mark.parametrize("kind", ["zero", "row0", "row239", "cols0_319"])
def test_frames_at_the_scans_edges(gh, depth, bufs, kind):
    """Each edge frame at positions 0, 1, middle and last of a 4-frame sequence: history rows
    (NaN after an empty frame) as the pipelined loop's, and the two buffers left behind as the
    host prepares them."""
    import hpe
    _set_params(gh.ctx, MAXITER)
    edge = _edge_frames(depth[0])[kind]
    for pos in range(4):
        frames = [d.copy() for d in depth[1:5]]
        frames[pos] = edge
        want = _pipelined(gh.ctx, frames, P_SEQ)
        hist, final = _raw_sequence(gh.ctx, _to_dev(frames), 4, P_SEQ, 3, bufs)
        assert np.array_equal(hist, want, equal_nan=True), (kind, pos)
        assert np.array_equal(final, want[-1], equal_nan=True), (kind, pos)
        for f in (3, 2):
            _check_buffer(gh.ctx.pipe_readback(f & 1), hpe.preprocess_depth(frames[f]))


def test_chunk_graphs_do_not_depend_on_sequence_length(depth, d_raw, bufs):
    """Chunks of 2 on a context of its own: a 7-frame sequence captures (2, parity 0, next) and
    (1, parity 0, last); a 5-frame one then captures nothing, though its chunk of frames 2, 3
    has no frame 5 to scan forward; a 4-frame one adds only (2, parity 0, last)."""
    import hpe
    hand = hpe.reference_hand(device=0)
    ctx = hand.ctx
    _set_params(ctx, MAXITER)
    want = _pipelined(ctx, depth, P_SEQ)
    seen = set()
    for n in (7, 5, 4):
        before = ctx.graph_captures()
        hist, final = _raw_sequence(ctx, d_raw, n, P_SEQ, 2, bufs)
        assert np.array_equal(hist, want[:n]), n
        assert np.array_equal(final, want[n - 1]), n
        shapes = {(min(2, n - f0), f0 & 1, f0 + 2 < n) for f0 in range(0, n, 2)}
        assert ctx.graph_captures() - before == len(shapes - seen), n
        seen |= shapes
    assert seen == {(2, 0, True), (1, 0, False), (2, 0, False)}
    ctx.close()


def test_prep_split_switch_off_same_bits(gh, depth, ref, tmp_path):
    """HPE_PREP_SPLIT=0 (read at hpe_create): a process with the switch tracks the same bits."""
    np.save(tmp_path / "frames.npy", np.stack(depth[:5]).astype(np.float32))
    env = dict(os.environ, HPE_PREP_SPLIT="0")
    subprocess.run([sys.executable, __file__, str(tmp_path / "frames.npy"), str(tmp_path / "out.npy"),
                    str(P_SEQ), str(MAXITER), "5", "2"], check=True, env=env, timeout=120)
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref[:5])


if __name__ == "__main__":
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root / "hand-pose-estimation_amd"), str(root / "oracle"), str(root / "tests")]
    import torch
    torch.cuda.is_available()  # torch's HIP runtime first, as conftest.py has it
    import hpe
    frames = np.load(sys.argv[1])
    P_, maxiter_, n_, K_ = (int(v) for v in sys.argv[3:7])
    hand = hpe.reference_hand(device=0)
    _set_params(hand.ctx, maxiter_)
    h_, _ = _raw_sequence(hand.ctx, _to_dev(list(frames)), n_, P_, K_, _buffers())
    np.save(sys.argv[2], h_)
    hand.ctx.close()
