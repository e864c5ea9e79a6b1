"""A context gives back what it took: create, touch every lazily allocated subsystem once at its
smallest shape, close -- four times over -- and device memory stops shrinking after the first
cycle, which warms the runtime (code objects, torch's and the library's own).

test_cycles_return_memory compares free device memory (torch.cuda.mem_get_info, read right after
a synchronise: other processes share the card) after cycle 4 with that after cycle 2.  The
context's members release themselves (csrc/hpe_own.hpp), so nothing a subsystem allocates can be
left off a list; this is the check that none is.

  PARENT_DROP: what the commit before the owners loses between those two readings, measured with
  this same file: 0 bytes in two runs out of two (readings after cycles 1..4: PARENT_READINGS,
  the same in both runs -- the first cycle's 16 MiB is the warm-up).  This commit measured 0
  bytes as well, with the same four readings, in two runs out of two (BRANCH_READINGS).
  GRANULE: one allocation granule of the driver as margin, 2 MiB (the size free memory moves by
  when a small hipMalloc opens a new block).

One cycle allocates tens of MiB in over a hundred buffers, the smallest of 4 bytes (a granule
when it opens a block), so a subsystem that stopped freeing would show as a multiple of the margin
only if it is large -- and every small one is still caught by the CPU check of the owners
(tests/test_own.py), which counts every allocation.

test_report_toggle_keeps_graphs: lane reports on (depth 2), off, on again on one context, a live
begin and a tracked frame after each.  The report buffers are allocated once, at the first set
that turns reports on, and never move, so the third begin's frame replays the first one's graph:
graph_captures() does not grow (PARENT_THIRD: 0 new captures at the commit before, where the
counter read 2, 4, 4 after the three batches, as it does at this one).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, MAXITER = 16, 3
PARENT_DROP = 0
GRANULE = 2 << 20
PARENT_THIRD = 0
PARENT_READINGS = (308363132928, 308346355712, 308346355712, 308346355712)
BRANCH_READINGS = (308363132928, 308346355712, 308346355712, 308346355712)


class Env:
    """What the cycles share: torch's buffers and the frames, made once, before any reading."""

    def __init__(self):
        import hpe
        import torch
        from hpe import synth, window
        self.hpe, self.torch, self.window = hpe, torch, window
        hand = hpe.reference_hand(device=0)
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        poses = synth.trajectory(2, seed=0)
        self.depth = [hand.ctx.render_depth(th) for th in poses]
        hand.ctx.close()
        self.obs = hpe.preprocess_depth(self.depth[0], True, True, 241.42)
        self.st = torch.zeros((2, 27), dtype=torch.float64, device="cuda:0")
        self.raw = torch.from_numpy(np.stack(self.depth)).to("cuda:0")
        self.rows = torch.zeros((2, 27), dtype=torch.float64)
        self.rows[:, :26] = torch.from_numpy(self.x0)
        torch.cuda.synchronize()

    def context(self):
        hand = self.hpe.reference_hand(device=0)
        ub, lb, sd = self.hpe.reference_bounds()
        pso = self.hpe.PSO()
        pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        pso._push(hand.ctx)
        return hand, hand.ctx

    def reset_states(self):
        self.st.copy_(self.rows)
        self.torch.cuda.synchronize()

    def free_bytes(self):
        self.torch.cuda.synchronize()
        return self.torch.cuda.mem_get_info()[0]


@pytest.fixture(scope="module")
def env():
    return Env()


def ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def cycle(env):
    hand, ctx = env.context()
    lib, d, o = ctx.lib, env.depth, env.obs
    sp = env.st.data_ptr()
    # store, select and prepare a frame
    ctx.store_frame(0, o["depth_cm"], o["dt"], o["cloud"], o["scale"], o["dtmax"], o["K"])
    ctx.select_frame(0)
    ctx.prepare_frame(1, d[0])
    ctx.prepare_frame(2, d[1])
    # pso_evolve and pso_optimise
    out, cost, tr = np.zeros(26), C.c_double(0), np.zeros(MAXITER - 1)
    ctx.check(lib.hpe_pso_evolve(ctx.h, ptr(env.x0), P, ptr(out), C.byref(cost)))
    ctx.check(lib.hpe_pso_optimise(ctx.h, ptr(env.x0), P, ptr(out), C.byref(cost), ptr(tr), MAXITER - 1))
    assert np.isfinite(cost.value)
    # the pipeline: begin and two frames
    env.reset_states()
    ctx.pipeline_begin(d[0])
    ctx.track_pipelined(P, 1, sp, d[1])
    ctx.track_pipelined(P, 1, sp, None)
    # a raw batch of two lanes, two frames
    env.reset_states()
    ctx.track_raw_batch(P, 1, sp, [env.raw.data_ptr()] * 2, 2)
    # a live batch of two lanes: reports, windows, one locate, two frames
    env.reset_states()
    ctx.set_batch_report(2)
    ctx.set_batch_window("fixed", [env.window.WHOLE] * 2)
    ctx.batch_pipeline_begin([d[0], d[0]])
    ctx.batch_pipeline_locate(sp, env.x0)
    ctx.track_batch_pipelined(P, 1, sp, [d[1], d[1]])
    ctx.track_batch_pipelined(P, 1, sp, None)
    assert ctx.batch_report_wait(0).seq == 2
    ctx.set_batch_window("off")
    ctx.set_batch_report(0)
    # pso_optimise of two lanes in the same launches
    env.reset_states()
    ctx.pso_optimise_batch(P, sp, [1, 2])
    ctx.check(lib.hpe_sync(ctx.h))
    assert np.isfinite(env.st.cpu().numpy()).all()
    # the scripted subswarm transport
    ctx.subswarm_init_scripted(np.zeros((2, 2, 27)), 0)
    ctx.subswarm_fini()
    # the profiling pools, the renderer, the pose rule, lane hands
    ctx.check(lib.hpe_profile_enable(ctx.h, 1))
    ctx.check(lib.hpe_profile_enable(ctx.h, 0))
    ctx.render_depth(env.x0)
    ctx.window_from_pose(env.x0)
    ctx.set_batch_hands([hand, hand])
    ctx.check(lib.hpe_sync(ctx.h))
    ctx.close()


def test_cycles_return_memory(env):
    free = []
    for _ in range(4):
        cycle(env)
        free.append(env.free_bytes())
    drop = free[1] - free[3]
    print(f"free device memory after cycles 1..4: {free}; cycle 2 -> 4 lost {drop} bytes")
    assert drop <= PARENT_DROP + GRANULE, (free, drop)


def test_report_toggle_keeps_graphs(env):
    hand, ctx = env.context()
    sp, d = env.st.data_ptr(), env.depth
    caps = []
    for depth in (2, 0, 2):
        ctx.set_batch_report(depth)
        env.reset_states()
        ctx.batch_pipeline_begin([d[0], d[0]])
        ctx.track_batch_pipelined(P, 1, sp, [d[1], d[1]])
        ctx.track_batch_pipelined(P, 1, sp, None)
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        assert np.isfinite(env.st.cpu().numpy()).all()
        if depth:
            assert ctx.batch_report_wait(1).seq == 2
        caps.append(ctx.graph_captures())
    ctx.close()
    print(f"graph captures after the three batches: {caps}")
    assert caps[1] > caps[0] > 0  # the batches do run as graphs, and reports are in their key
    assert caps[2] - caps[1] <= PARENT_THIRD, caps
