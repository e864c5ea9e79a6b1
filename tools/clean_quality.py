"""What lane cleaning buys on one noisy stream (hpe_set_batch_clean): one synthetic sequence
(hpe.synth.trajectory seed 0, 256 particles, 30 generations, refine on), quantised to 16 bits at
--unit mm per count and passed through hpe.synth.camera_noise (flying pixels on the silhouette,
speckle around the hand), tracked as a one-lane live u16 batch three ways:
  raw            the noisy frames as they are;
  device         the noisy frames, cleaned by the batch with the default parameters;
  host mirror    the noisy frames cleaned by hpe.clean on the host, fed to the uncleaned batch.
Each is compared with the tracked poses of the noise-free stream (the same batch on the quantised
renders): the mean absolute difference over the 26 parameters and all frames (cm and radians
mixed, as the reference's theta), and the largest.  device and host mirror must agree bit for bit.

Prints one JSON line per run.
Usage (GPU box): python tools/clean_quality.py [--frames 48] [--unit 1.0] [--background 800]
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "hand-pose-estimation_amd")]

import numpy as np  # noqa: E402

P, G = 256, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--unit", type=float, default=1.0, metavar="MM")
    ap.add_argument("--background", type=float, default=800.0, metavar="MM")
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import hpe
    from hpe import clean, synth
    n, unit = a.frames, np.float32(a.unit)
    ctx = hpe.reference_hand(device=0).ctx
    ub, lb, sd = hpe.reference_bounds()
    pso = hpe.PSO()
    pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, G + 1, 1e-8, 1e-8)
    pso._push(ctx)
    truth = np.asarray(synth.trajectory(n, 0, revert=0.02), dtype=np.float64)
    q = [np.rint(np.asarray(ctx.render_depth(th), dtype=np.float32) / unit).clip(0, 65535)
         .astype(np.uint16) for th in truth]
    noisy = [synth.camera_noise(f, k, background=int(a.background / unit), jitter=int(30 / unit))
             for k, f in enumerate(q)]
    par = clean.defaults(float(unit))
    mirror = [par.apply(f) for f in noisy]
    st = torch.zeros((1, 27), dtype=torch.float64, device="cuda:0")

    def track(frames, params):
        x0 = np.zeros((1, 27))
        x0[0, :26] = hpe.X0
        st.copy_(torch.from_numpy(x0))
        torch.cuda.synchronize()
        rows = []
        ctx.set_batch_clean(params)
        try:
            ctx.batch_pipeline_begin([frames[0]], input="u16", unit_mm=float(unit))
            for f in range(n):
                ctx.track_batch_pipelined(P, 1, st.data_ptr(), [frames[f + 1]] if f + 1 < n else None)
                ctx.check(ctx.lib.hpe_sync(ctx.h))
                rows.append(st.cpu().numpy()[0].copy())
        finally:
            ctx.set_batch_clean(None)
        return np.array(rows)

    base = track(q, None)
    runs = {"noise-free": base, "raw": track(noisy, None), "device": track(noisy, [par]),
            "host mirror": track(mirror, None)}
    changed = [int((m != f).sum()) for m, f in zip(mirror, noisy)]
    injected = [int((f != g).sum()) for f, g in zip(noisy, q)]
    for name, rows in runs.items():
        err = np.abs(rows[:, :26] - base[:, :26])
        print(json.dumps({
            "run": name, "frames": n, "unit_mm": float(unit), "edge": par.edge,
            "support": par.support, "median": par.median,
            "mean_abs_pose_err_vs_noise_free": float(err.mean()),
            "max_abs_pose_err_vs_noise_free": float(err.max()),
            "mean_abs_pose_err_vs_true_pose": float(np.abs(rows[:, :26] - truth).mean()),
            "mean_cost": float(rows[:, 26].mean()),
            "injected_pixels_per_frame": float(np.mean(injected)),
            "pixels_cleaning_changes_per_frame": float(np.mean(changed)),
            "rows_sha1": hashlib.sha1(rows.tobytes()).hexdigest()[:16]}), flush=True)
    same = bool(np.array_equal(runs["device"], runs["host mirror"]))
    print(json.dumps({"device_equals_host_mirror": same}), flush=True)
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
