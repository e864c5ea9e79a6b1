"""What a lane group buys on one stream (hpe_set_batch_seeds + hpe_set_batch_groups): one 16-lane
wave-form group of 256-particle subswarms, seeds 1000..1015, against a single context at 4096
particles and against one ungrouped 256-particle lane, on the same resident raw frames of one
synthetic sequence (hpe.synth.trajectory seed 0, 30 generations, refine on, N = 250).

Prints one JSON line per form: tracked frames/s of the stream (median of --reps timed runs after
one that captures the graphs), and per frame the final cost and the pose error against the
trajectory's true pose -- the mean absolute difference over the 26 parameters (cm and radians
mixed, as the reference's theta) and the largest.
Usage (GPU box): python tools/group_quality.py [--frames 48] [--reps 3] [--lanes 16]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "hand-pose-estimation_amd")]

import numpy as np  # noqa: E402

G, FPG = 30, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=16)
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import hpe
    from hpe import synth
    n, B = a.frames, a.lanes
    ctx = hpe.reference_hand(device=0).ctx
    ub, lb, sd = hpe.reference_bounds()
    pso = hpe.PSO()
    pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, G + 1, 1e-8, 1e-8)
    pso._push(ctx)
    truth = np.asarray(synth.trajectory(n, 0, revert=0.02), dtype=np.float64)
    raw = torch.from_numpy(np.stack([np.ascontiguousarray(ctx.render_depth(th), dtype=np.float32)
                                     for th in truth])).to("cuda:0")

    def measure(name, lanes, run, extra):
        x0 = np.zeros((lanes, 27))
        x0[:, :26] = hpe.X0
        st = torch.from_numpy(x0).to("cuda:0")
        hist = torch.empty((lanes, n, 27), dtype=torch.float64, device="cuda:0")
        times = []
        for _ in range(a.reps + 1):  # the first call captures the graphs
            st.copy_(torch.from_numpy(x0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(st, hist)
            ctx.check(ctx.lib.hpe_sync(ctx.h))
            times.append(time.perf_counter() - t0)
        h = hist.cpu().numpy()[0]  # lane 0 carries the stream's row (a group's lanes all do)
        err = np.abs(h[:, :26] - truth)
        line = {"form": name, "frames": n, "reps": a.reps,
                "stream_fps": n / float(np.median(times[1:])),
                "stream_fps_runs": [n / t for t in times[1:]],
                "mean_cost": float(h[:, 26].mean()), "last_cost": float(h[-1, 26]),
                "mean_abs_pose_err": float(err.mean()), "max_abs_pose_err": float(err.max()),
                "cost_per_frame": [round(float(v), 4) for v in h[:, 26]],
                "mean_abs_pose_err_per_frame": [round(float(v), 5) for v in err.mean(axis=1)]}
        line.update(extra)
        print(json.dumps(line), flush=True)

    # one ungrouped 256-particle lane, wave form
    ctx.set_batch_form("wave")
    measure("one lane, 256 p, wave form", 1,
            lambda st, hist: ctx.track_raw_batch(256, 1, st.data_ptr(), [raw.data_ptr()], n,
                                                 frames_per_graph=FPG, d_hist_ptr=hist.data_ptr()),
            {"lanes": 1})
    # the group: B lanes over the one stream, seeds 1000 + b
    ctx.set_batch_seeds([1000 + b for b in range(B)])
    ctx.set_batch_groups([B])
    measure("group of %d lanes x 256 p, wave form" % B, B,
            lambda st, hist: ctx.track_raw_batch(256, 1, st.data_ptr(), [raw.data_ptr()] * B, n,
                                                 frames_per_graph=FPG, d_hist_ptr=hist.data_ptr()),
            {"lanes": B, "wpp": ctx.batch_wave_wpp(256, B)})
    # the same lanes ungrouped: independent subswarms that never exchange
    ctx.set_batch_groups(None)
    measure("%d independent lanes x 256 p (lane 0 shown), wave form" % B, B,
            lambda st, hist: ctx.track_raw_batch(256, 1, st.data_ptr(), [raw.data_ptr()] * B, n,
                                                 frames_per_graph=FPG, d_hist_ptr=hist.data_ptr()),
            {"lanes": B})
    ctx.set_batch_seeds(None)
    ctx.set_batch_form("auto")
    # one swarm of B * 256 particles on a single context (the wave form from 1024 particles up)
    measure("single sequence, %d p" % (B * 256), 1,
            lambda st, hist: ctx.track_raw_sequence(B * 256, 1, st.data_ptr(), raw.data_ptr(), n,
                                                    frames_per_graph=FPG, d_hist_ptr=hist.data_ptr()),
            {"lanes": 0})
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
