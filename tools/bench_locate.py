"""Time lane location (hpe_batch_pipeline_locate) at 1 / 4 / 16 lanes, float and u16 frames, against
the course open without it, in one session with alternating legs:

  (a) locate   on a live batch begun with whole-frame windows: --calls consecutive calls (three
               launches each: locate, the found lanes' preparation again, the placement) between
               two events on the context's stream, device time per call -- one call alone is a
               third of a millisecond, too short a window for one bracket -- and the host clock
               around ONE call and an hpe_sync, what a caller that waits for the result sees;
  (b) device   the whole first-frame course with it: hpe_set_batch_window(whole frames), begin,
               locate, hpe_sync -- host clock;
  (c) host     the course open before: every lane's frame located on the host by the numpy mirror
               (hpe.locate.locate; the application holds the frames), the rows placed with
               hpe_build_spheres, the rows uploaded, hpe_set_batch_window(the located windows),
               begin, hpe_sync -- host clock.  A window cannot change while a batch lives, so for
               a lane that is LOST mid-batch this course also means ending the batch.

(c) is numpy, not a tuned host implementation: the line reports the mirror's share of it so that
the reader can put a faster host routine in its place.  Each leg runs once discarded, then --runs
times; medians and extremes, one JSON line per (lanes, format), appended to --out.  The results of
(b) and (c) are compared bit for bit (windows and rows).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "hand-pose-estimation_amd")]
import torch  # noqa: E402  (HIP runtime first)

torch.cuda.init()
import numpy as np  # noqa: E402

import hpe  # noqa: E402
from hpe import _lib, locate, synth, window  # noqa: E402

FOCAL, UNIT = 241.42, 0.25


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--lanes", default="1,4,16")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="locate calls per event bracket")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_locate" / "bench_locate.jsonl"))
    a = ap.parse_args()
    lanes = [int(x) for x in a.lanes.split(",")]
    if a.runs < 1 or a.calls < 1 or any(not 1 <= b <= _lib.BATCH_MAX for b in lanes):
        ap.error("--runs >= 1 and lanes in 1..%d" % _lib.BATCH_MAX)
    hand = hpe.reference_hand(device=0)
    ctx = hand.ctx
    Bmax = max(lanes)
    scenes = []
    for b in range(Bmax):  # lane b: a hand of its own in front of a wall, with forearm and speckle
        th = synth.trajectory(3, seed=b)[-1]
        th[3] += (b % 5 - 2) * 2.0
        scenes.append(synth.rig_scene(ctx.render_depth(th), th[3:6], FOCAL, seed=b))
    frames = {"f32": scenes, "u16": [np.round(s / np.float32(UNIT)).astype(np.uint16) for s in scenes]}
    T = np.asarray(hpe.X0, dtype=np.float64)
    stream = torch.cuda.ExternalStream(ctx.lib.hpe_stream(ctx.h))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)

    def sync():
        ctx.check(ctx.lib.hpe_sync(ctx.h))

    def end(st):  # a window cannot be set while a batch lives: the track call that ends it
        ctx.track_batch_pipelined(32, 0, st.data_ptr(), None)
        sync()

    ub, lb, sd = hpe.reference_bounds()
    pso = hpe.PSO()
    pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, 2, 1e-8, 1e-8)
    pso._push(ctx)
    for B in lanes:
        for inp in ("f32", "u16"):
            fr = frames[inp][:B]
            unit = UNIT if inp == "u16" else None
            st = torch.zeros((B, 27), dtype=torch.float64, device="cuda:0")
            legs = {"locate_dev": [], "locate_host": [], "device_course": [], "host_course": [],
                    "host_mirror": []}
            same = True
            for r in range(a.runs + 1):  # run 0 is the discarded warm-up of every leg
                # (b) the device course, and (a) inside it
                st.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.set_batch_window("fixed", [window.WHOLE] * B)
                ctx.batch_pipeline_begin(fr, input=inp, unit_mm=UNIT)
                ctx.batch_pipeline_locate(st.data_ptr(), T)
                sync()
                dev_course = (time.perf_counter() - t0) * 1e3
                rows_d, wins_d = st.cpu().numpy()[:, :26], ctx.batch_windows_readback(0, B)
                t0 = time.perf_counter()
                ctx.batch_pipeline_locate(st.data_ptr(), T)
                sync()
                loc_host = (time.perf_counter() - t0) * 1e3
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    ctx.batch_pipeline_locate(st.data_ptr(), T)
                e1.record(stream)
                sync()
                e1.synchronize()
                loc_dev = e0.elapsed_time(e1) / a.calls
                end(st)
                # (c) the host course
                st.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = [locate.locate(f, FOCAL, unit_mm=unit) for f in fr]
                mirror = (time.perf_counter() - t0) * 1e3
                S = locate.camera_centres(hand.build_batch(T)[0][0])
                rows = np.zeros((B, 27))
                rows[:, :26] = [locate.place(S, T, q.centre) if q.found else T for q in res]
                st.copy_(torch.from_numpy(rows))
                ctx.set_batch_window("fixed", [q.window if q.found else window.WHOLE for q in res])
                ctx.batch_pipeline_begin(fr, input=inp, unit_mm=UNIT)
                sync()
                host_course = (time.perf_counter() - t0) * 1e3
                rows_h, wins_h = st.cpu().numpy()[:, :26], ctx.batch_windows_readback(0, B)
                end(st)
                same = same and np.array_equal(rows_d, rows_h) and wins_d == wins_h
                if r:
                    legs["locate_dev"].append(loc_dev)
                    legs["locate_host"].append(loc_host)
                    legs["device_course"].append(dev_course)
                    legs["host_course"].append(host_course)
                    legs["host_mirror"].append(mirror)
            line = {"bench": "locate", "B": B, "input": inp, "calls_per_bracket": a.calls, "found": int(sum(q.found for q in res)),
                    "device_equals_host": bool(same)}
            line.update({k: stats(v) for k, v in legs.items()})
            line["course_speedup"] = line["host_course"]["median_ms"] / line["device_course"]["median_ms"]
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
