"""B independent sequences tracked in the same launches (hpe_track_batch_dev): one context, one
stream, one captured graph per chunk of frames for all lanes -- a generation launch covers
B x 256 particles, a refine launch is B workgroups.

Every lane has its own synthetic sequence (seeds 0..B-1, as tools/serve_streams.py makes them),
device-prepared into resident slots.  First checks on 6 frames that every lane of a batch
equals the same lane tracked alone by track_sequence, bit for bit; then prints one JSON line
per lane count with the aggregate tracked frames/s and the time of one batched frame.
Usage (GPU box): python tools/bench_batch.py [--lanes 1,2,4,8,16] [--frames 48] [--reps 3]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "hand-pose-estimation_amd")]

import numpy as np  # noqa: E402

P, G, FPG = 256, 30, 8


def make_lanes(ctx, B, n):
    """Lane b's n frames rendered and prepared into slots b n .. b n + n - 1."""
    from hpe import synth
    for b in range(B):
        poses = synth.trajectory(n, b, revert=0.02)
        for f, th in enumerate(poses):
            ctx.prepare_frame(b * n + f, np.ascontiguousarray(ctx.render_depth(th)))
    ctx.check(ctx.lib.hpe_sync(ctx.h))


def start_states(torch, x0, B):
    x = np.zeros((B, 27))
    x[:, :26] = x0
    return torch.from_numpy(x).to("cuda:0")


def check_against_alone(ctx, torch, x0, B, n_frames, n=6):
    st = start_states(torch, x0, B)
    hist = torch.empty((B, n, 27), dtype=torch.float64, device="cuda:0")
    ctx.track_batch(P, 1, st.data_ptr(), [b * n_frames for b in range(B)], n, FPG, hist.data_ptr())
    ctx.check(ctx.lib.hpe_sync(ctx.h))
    s1 = torch.empty(27, dtype=torch.float64, device="cuda:0")
    h1 = torch.empty((n, 27), dtype=torch.float64, device="cuda:0")
    for b in range(B):
        s1.copy_(start_states(torch, x0, 1)[0])
        ctx.track_sequence(P, 1, s1.data_ptr(), b * n_frames, n, FPG, h1.data_ptr())
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        if not (np.array_equal(h1.cpu().numpy(), hist[b].cpu().numpy())
                and np.array_equal(s1.cpu().numpy(), st[b].cpu().numpy())):
            raise AssertionError(f"lane {b} of the batch differs from the lane tracked alone")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", default="1,2,4,8,16")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import hpe
    counts = [int(x) for x in a.lanes.split(",")]
    n = a.frames
    hand = hpe.reference_hand(device=0)
    ctx = hand.ctx
    ub, lb, sd = hpe.reference_bounds()
    pso = hpe.PSO()
    pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, G + 1, 1e-8, 1e-8)
    pso._push(ctx)
    make_lanes(ctx, max(counts), n)
    check_against_alone(ctx, torch, hpe.X0, min(3, max(counts)), n)
    for B in counts:
        slots = [b * n for b in range(B)]
        st = start_states(torch, hpe.X0, B)
        x0 = st.clone()
        times = []
        for rep in range(a.reps + 1):  # the first call captures the graphs
            st.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.track_batch(P, 1, st.data_ptr(), slots, n, FPG)
            ctx.check(ctx.lib.hpe_sync(ctx.h))
            times.append(time.perf_counter() - t0)
        el = float(np.median(times[1:]))
        print(json.dumps({"lanes": B, "frames_per_lane": n, "reps": a.reps,
                          "aggregate_tracked_fps": B * n / el,
                          "ms_per_batched_frame": el / n * 1e3,
                          "workload": "256 p x 30 gen, refine on, N = 250, resident prepared "
                                      "frames, 8 frames per graph, one context, seeds 0..B-1"}),
              flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
