"""B independent sequences tracked in the same launches (hpe_track_batch_dev): one context, one
stream, one captured graph per chunk of frames for all lanes -- a generation launch covers
B x 256 particles, a refine launch is B workgroups.

Every lane has its own synthetic sequence (seeds 0..B-1, as tools/serve_streams.py makes them),
device-prepared into resident slots.  First checks on 6 frames that every lane of a batch
equals the same lane tracked alone by track_sequence, bit for bit; then prints one JSON line
per lane count with the aggregate tracked frames/s and the time of one batched frame.
--raw: the same lane counts and workload over raw float mm frames resident in HBM
(hpe_track_raw_batch_dev: every lane's next frame is prepared inside the lanes' refine launch);
the check is then against track_raw_sequence alone.  --live: the same lanes and workload fed a
frame per lane and call from host memory (hpe_batch_pipeline_begin / hpe_track_batch_pipelined:
one graph per frame, the next frames read from pinned host buffers inside the refine launch);
the check is then against the single pipelined loop (track_pipelined) alone.  --profile adds the mean device time of the
refine, init, generation and final kernels of one more pass (HPE_PROF_*, direct launches).
--form wave (with any mode): the lanes' pso_evolve in the wave-per-particle form
(hpe_set_batch_form); every line then carries the form and the waves per particle its launches
used (hpe_batch_wave_wpp), and the check is against the single call on a second context created
under HPE_PSO_FORM=wave and HPE_PSO_WPP=<the checked batch's>.
--window fixed|follow (with --raw or --live): the lanes' frames read through lane windows
(hpe_set_batch_window).  fixed: whole-frame windows, so the line prices the masking alone;
follow: windows re-centred on the device from every lane's tracked pose, with margins (8 cm) wide
enough that nothing is cut on the synthetic streams, so the line prices the masking and the
window launch per frame.  The check against the lanes alone runs without windows; every line then
records whether the timed run's results (raw: the histories; live: the final states) equalled a
run of the same lanes without windows ("equals_off": informational, not asserted).
--hands distinct (with any mode and form): a hand model per lane (hpe_set_batch_hands) -- lane b
of a B-lane line tracks frames rendered with its own hpe.scaled_hand(0.9 + 0.2 b / max(B - 1, 1))
under that hand; the default, shared, is every lane on the context's hand.  Each line is then
checked first (6 frames, every lane against the single call on its own hand's context; under
--form wave on the first line only, whose yardstick contexts are created in that form).
--pacing free (with --live): the live batch under hpe_set_batch_pacing(HPE_PACING_FREE), the
idle-aware kernel forms; without --drop every lane still gives every frame, so the line prices the
forms' entry test and the per-call activity write against --pacing lockstep.
--drop K (with --live): a staggered drop of one frame in K per lane -- lane b gives no frame in
the next-frame array of every call whose index is = b mod K (the begin takes a frame of every
lane).  Under --pacing free that lane idles for the following call.  Under --pacing lockstep the
tool does what a caller has to do without pacing: whenever the set of lanes with a frame changes it
ends the batch and begins another of just those lanes, their state rows gathered into a dense
buffer and scattered back.  Both lines count the frames actually tracked ("tracked_frames").
--report DEPTH (with --live): lane reports on (hpe_set_batch_report), a ring of DEPTH per lane, so
the line prices the report launch per frame against a run without it.
--consume sync|report (with --live): the application reads every frame's result -- sync: what it
does without reports, hpe_sync and a device-to-host copy of the B x 27 states after every call;
report (needs --report): each lane's newest report after every call, one call behind, never
synchronising.  "results_consumed" counts the rows / complete reports read.
--input f32|u16, --unit MM (with --live): the lanes' frame format.  --input u16 or any --unit
quantises the rendered frames once, np.rint(render / unit) as uint16 (unit default 1 mm); a u16
run feeds those (hpe_batch_pipeline_begin_u16), the matching f32 run (--input f32 --unit MM)
hpe.depth_u16_to_mm of the same frames, so both track identical trajectories, do identical device
work and print the same results_sha1.  Without either option the rendered floats are fed as ever.
--in-place (with --live): every next frame is written into the lane's pinned buffer
(hpe_batch_frame_buffer) and that buffer passed back, so the library copies nothing; the write is
the tool's, standing in for the camera's.  Every --live line names its "input" and "in_place",
and "host_bytes_copied_per_call", the bytes the library copies into the ring per call.
--input view --cam WxH --step K (with --live): the lanes deliver 16-bit frames at the camera's own
resolution, read through a lane view (hpe_batch_pipeline_begin_view) -- the centred view of that
step, hpe.view.View(W, H, W, (H - 240 K) // 2, (W - 320 K) // 2, K).  A camera frame is the
quantised rendered frame enlarged K times (every camera pixel of a model pixel's block holds its
value) on an empty canvas; the check asserts that the mirror (View.reduce) gives the quantised
frame back, and runs the lanes alone on its float conversion.  --host-reduce (with --input u16 and
--cam): the same camera frames, reduced by the tool inside the timed loop with the strided copy an
application makes without views, cam[r0:r0+240K:K, c0:c0+320K:K], and fed to the plain u16 batch
(with --in-place that copy goes straight into the lane's pinned buffer): the baseline a view batch
is measured against.  All three runs track identical trajectories and print the same results_sha1.
--clean (with --live --input u16|view): lane cleaning on (hpe_set_batch_clean) with the default
parameters of the run's unit in every lane, set after the check; the line carries "clean": true
and prices the cleaning launch per frame against a run without it (the frames are the noise-free
renders: the median still moves silhouette values, so results_sha1 differs from the run without).
--seeds distinct (with any mode and form): a seed per lane (hpe_set_batch_seeds), lane b's 1000 + b;
the default, shared, is every lane under the context's seed (the call is not made).  The check
against the lanes alone runs before the seeds are set.
--group N (with any mode and form; N divides every lane count): groups of N consecutive lanes over
one stream (hpe_set_batch_groups) -- lane b is fed stream b // N, and after every frame the group's
rows become its best own row.  Every line then carries "group", and "final_cost", the cost of
every lane's row after the last frame.
Usage (GPU box): python tools/bench_batch.py [--raw | --live] [--form auto|wave] [--profile]
                                             [--seeds shared|distinct] [--group N]
                                             [--window off|fixed|follow] [--hands shared|distinct]
                                             [--pacing lockstep|free] [--drop K]
                                             [--report DEPTH] [--consume sync|report]
                                             [--input f32|u16|view] [--unit MM] [--in-place]
                                             [--cam WxH] [--step K] [--host-reduce] [--clean]
                                             [--lanes 1,2,4,8,16] [--frames 48] [--reps 3]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "hand-pose-estimation_amd")]

import numpy as np  # noqa: E402

P, G, FPG = 256, 30, 8
WIN_MARGIN = 8.0  # cm, --window follow: nothing of the synthetic hands is cut


def lane_scale(b, B):
    """--hands distinct: the size of lane b's hand, 0.9 .. 1.1 over the lanes."""
    return 0.9 + 0.2 * b / max(B - 1, 1)


def make_lanes(ctx, B, n, render=None):
    """Lane b's n frames rendered (by render[b], default ctx) and prepared into slots
    b n .. b n + n - 1."""
    from hpe import synth
    for b in range(B):
        poses = synth.trajectory(n, b, revert=0.02)
        r = render[b] if render else ctx
        for f, th in enumerate(poses):
            ctx.prepare_frame(b * n + f, np.ascontiguousarray(r.render_depth(th)))
    ctx.check(ctx.lib.hpe_sync(ctx.h))


def make_raw_lanes(ctx, torch, B, n, render=None):
    """Lane b's n frames rendered (by render[b], default ctx) and uploaded as one raw device
    tensor (n x 240 x 320 float mm)."""
    from hpe import synth
    out = []
    for b in range(B):
        poses = synth.trajectory(n, b, revert=0.02)
        r = render[b] if render else ctx
        fr = np.stack([np.ascontiguousarray(r.render_depth(th)) for th in poses])
        out.append(torch.from_numpy(fr.astype(np.float32)).to("cuda:0"))
    return out


def start_states(torch, x0, B):
    x = np.zeros((B, 27))
    x[:, :26] = x0
    return torch.from_numpy(x).to("cuda:0")


def wave_yardstick_context(hpe, pso, wpp, scale=None):
    """A second context for the single calls a wave-form batch is checked against: the wave form
    at the batch's waves per particle (both read from the environment at hpe_create); with the
    reference hand, or scaled_hand(scale)."""
    saved = {k: os.environ.get(k) for k in ("HPE_PSO_FORM", "HPE_PSO_WPP")}
    os.environ.update(HPE_PSO_FORM="wave", HPE_PSO_WPP=str(wpp))
    try:
        hand = hpe.reference_hand(device=0) if scale is None else hpe.scaled_hand(scale)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    pso._push(hand.ctx)
    return hand


def lane_alone(alone, b):
    """The yardstick context of lane b: alone is one context for every lane, or one per lane."""
    return alone[b] if isinstance(alone, (list, tuple)) else alone


def check_against_alone(ctx, torch, x0, B, n_frames, n=6, alone=None):
    st = start_states(torch, x0, B)
    hist = torch.empty((B, n, 27), dtype=torch.float64, device="cuda:0")
    ctx.track_batch(P, 1, st.data_ptr(), [b * n_frames for b in range(B)], n, FPG, hist.data_ptr())
    ctx.check(ctx.lib.hpe_sync(ctx.h))
    s1 = torch.empty(27, dtype=torch.float64, device="cuda:0")
    h1 = torch.empty((n, 27), dtype=torch.float64, device="cuda:0")
    for b in range(B):
        ctx = lane_alone(alone, b) or ctx
        s1.copy_(start_states(torch, x0, 1)[0])
        ctx.track_sequence(P, 1, s1.data_ptr(), b * n_frames, n, FPG, h1.data_ptr())
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        if not (np.array_equal(h1.cpu().numpy(), hist[b].cpu().numpy())
                and np.array_equal(s1.cpu().numpy(), st[b].cpu().numpy())):
            raise AssertionError(f"lane {b} of the batch differs from the lane tracked alone")


def check_raw_against_alone(ctx, torch, x0, raws, n=6, alone=None):
    B = len(raws)
    st = start_states(torch, x0, B)
    hist = torch.empty((B, n, 27), dtype=torch.float64, device="cuda:0")
    ctx.track_raw_batch(P, 1, st.data_ptr(), [r.data_ptr() for r in raws], n,
                        frames_per_graph=FPG, d_hist_ptr=hist.data_ptr())
    ctx.check(ctx.lib.hpe_sync(ctx.h))
    s1 = torch.empty(27, dtype=torch.float64, device="cuda:0")
    h1 = torch.empty((n, 27), dtype=torch.float64, device="cuda:0")
    for b in range(B):
        ctx = lane_alone(alone, b) or ctx
        s1.copy_(start_states(torch, x0, 1)[0])
        ctx.track_raw_sequence(P, 1, s1.data_ptr(), raws[b].data_ptr(), n, frames_per_graph=FPG,
                               d_hist_ptr=h1.data_ptr())
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        if not (np.array_equal(h1.cpu().numpy(), hist[b].cpu().numpy())
                and np.array_equal(s1.cpu().numpy(), st[b].cpu().numpy())):
            raise AssertionError(f"lane {b} of the raw batch differs from the lane tracked alone")


def make_host_lanes(ctx, B, n):
    """Lane b's n frames rendered into host memory (float mm 240 x 320 each)."""
    from hpe import synth
    return [[np.ascontiguousarray(ctx.render_depth(th), dtype=np.float32)
             for th in synth.trajectory(n, b, revert=0.02)] for b in range(B)]


def next_in_place(ctx, host, f, reduce=None):
    """Frame f of every lane written into the lane's pinned buffer of the next call: the buffers,
    to be passed back as the call's next frames.  reduce: the strided view of a camera frame that
    is written instead (--host-reduce: the copy into the buffer is the reduction)."""
    out = []
    for b, fr in enumerate(host):
        buf = ctx.batch_frame_buffer(b)
        buf[:] = fr[f] if reduce is None else reduce(fr[f])
        out.append(buf)
    return out


def lanes_kw(begin_kw, B):
    """The begin's keywords for B lanes: one view for every lane becomes B views."""
    kw = dict(begin_kw or {})
    if "views" in kw:
        kw["views"] = [kw["views"]] * B
    return kw


def run_live(ctx, st, host, n, consume=None, begin_kw=None, in_place=False, reduce=None):
    """n frames of every lane of host through the live batch, a frame per lane and call
    (begin_kw: the begin's input format; in_place: next_in_place instead of arrays to copy;
    reduce: --host-reduce, every camera frame reduced by the tool before it is given).
    consume "sync": after every call hpe_sync and a device-to-host copy of the B x 27 states (what
    an application does without reports); "report": after every call each lane's newest report is
    read, one call behind and without any synchronisation (--report), and the last ones at the
    end.  Returns the results consumed: the number of state rows or complete reports read."""
    B, got = len(host), 0
    give = (lambda x: x) if reduce is None else (lambda x: np.ascontiguousarray(reduce(x)))
    ctx.batch_pipeline_begin([give(fr[0]) for fr in host], **lanes_kw(begin_kw, B))
    for f in range(n):
        if f + 1 >= n:
            nxt = None
        elif in_place:
            nxt = next_in_place(ctx, host, f + 1, reduce)
        else:
            nxt = [give(fr[f + 1]) for fr in host]
        ctx.track_batch_pipelined(P, 1, st.data_ptr(), nxt)
        if consume == "sync":
            ctx.check(ctx.lib.hpe_sync(ctx.h))
            got += len(st.cpu().numpy())
        elif consume == "report":
            got += sum(ctx.batch_report(b, raw=True).seq > 0 for b in range(B))
    if consume == "report":
        got += sum(ctx.batch_report_wait(b, 0, 5000, raw=True).seq == n for b in range(B))
    return got


def gives(b, step, K):
    """--drop K: whether lane b gives a frame at step `step` (0: the begin, s >= 1: the next-frame
    array of call s - 1)."""
    return not K or step == 0 or (step - 1) % K != b % K


def run_live_paced(ctx, st, host, n, K):
    """n steps of a free-paced batch under --drop K: every lane takes its frames in order, and
    idles in the call after a step it gave no frame at.  Returns the frames tracked."""
    B = len(host)
    took = [0] * B

    def frames(step):
        fr = [None] * B
        for b in range(B):
            if gives(b, step, K):
                fr[b] = host[b][took[b]]
                took[b] += 1
        return fr

    ctx.batch_pipeline_begin(frames(0))
    for s in range(n):
        ctx.track_batch_pipelined(P, 1, st.data_ptr(), frames(s + 1) if s + 1 < n else None)
    return sum(took)


def run_live_rebegin(ctx, torch, st, subs, host, n, K):
    """The same schedule without pacing: a lockstep batch of just the lanes that have a frame,
    ended and begun again whenever that set changes (state rows gathered into subs[len(set)] and
    scattered back).  Returns the frames tracked."""
    B = len(host)
    took = [0] * B

    def frames(A):
        fr = [host[b][took[b]] for b in A]
        for b in A:
            took[b] += 1
        return fr

    s = 0
    while s < n:
        A = [b for b in range(B) if gives(b, s, K)]
        e = s
        while e + 1 < n and [b for b in range(B) if gives(b, e + 1, K)] == A:
            e += 1
        idx = torch.tensor(A, device="cuda:0")
        sub = subs[len(A)]
        sub.copy_(st[idx])
        ctx.batch_pipeline_begin(frames(A))
        for q in range(s, e + 1):
            ctx.track_batch_pipelined(P, 1, sub.data_ptr(), frames(A) if q < e else None)
        st[idx] = sub
        s = e + 1
    return sum(took)


def check_live_against_alone(ctx, torch, x0, host, n=6, alone=None, feed=None, begin_kw=None,
                             in_place=False, reduce=None):
    """host: the lanes' float frames, which the lanes alone track; feed: what the batch is given
    (default: host; the u16 frames that host converts, for a u16 batch; camera frames for a view
    batch, or with reduce, the tool's own reduction, for --host-reduce)."""
    B = len(host)
    feed = host if feed is None else feed
    st = start_states(torch, x0, B)
    hist = []
    give = (lambda x: x) if reduce is None else (lambda x: np.ascontiguousarray(reduce(x)))
    ctx.batch_pipeline_begin([give(fr[0]) for fr in feed], **lanes_kw(begin_kw, B))
    for f in range(n):
        if f + 1 >= n:
            nxt = None
        elif in_place:
            nxt = next_in_place(ctx, feed, f + 1, reduce)
        else:
            nxt = [give(fr[f + 1]) for fr in feed]
        ctx.track_batch_pipelined(P, 1, st.data_ptr(), nxt)
        ctx.check(ctx.lib.hpe_sync(ctx.h))
        hist.append(st.cpu().numpy().copy())
    s1 = torch.empty(27, dtype=torch.float64, device="cuda:0")
    for b in range(B):
        ctx = lane_alone(alone, b) or ctx
        s1.copy_(start_states(torch, x0, 1)[0])
        ctx.pipeline_begin(host[b][0])
        for f in range(n):
            ctx.track_pipelined(P, 1, s1.data_ptr(), host[b][f + 1] if f + 1 < n else None)
            ctx.check(ctx.lib.hpe_sync(ctx.h))
            if not np.array_equal(s1.cpu().numpy(), hist[f][b]):
                raise AssertionError(f"lane {b}, frame {f} of the live batch differs from the "
                                     "lane tracked alone")


def kernel_means_us(ctx, run):
    """Mean device microseconds per launch of the profiled kernels over one pass of run()."""
    from hpe import _lib
    ctx.check(ctx.lib.hpe_profile_enable(ctx.h, 1))
    run()
    out = {}
    for name, kid in (("refine", _lib.PROF_REFINE), ("init", _lib.PROF_PSO_INIT),
                      ("gen", _lib.PROF_PSO_GEN), ("final", _lib.PROF_PSO_FINAL)):
        nl = C.c_int32(0)
        tot, mn, mx = C.c_double(0), C.c_double(0), C.c_double(0)
        ctx.check(ctx.lib.hpe_profile_read_kernel(ctx.h, kid, C.byref(nl), C.byref(tot),
                                                  C.byref(mn), C.byref(mx)))
        out[name] = {"launches": nl.value, "mean_us": tot.value / max(nl.value, 1) * 1e3}
    ctx.check(ctx.lib.hpe_profile_enable(ctx.h, 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", default="1,2,4,8,16")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--raw", action="store_true")
    ap.add_argument("--live", action="store_true")
    ap.add_argument("--form", choices=("auto", "wave"), default="auto")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--window", choices=("off", "fixed", "follow"), default="off")
    ap.add_argument("--hands", choices=("shared", "distinct"), default="shared")
    ap.add_argument("--pacing", choices=("lockstep", "free"), default="lockstep")
    ap.add_argument("--drop", type=int, default=0)
    ap.add_argument("--report", type=int, default=0, metavar="DEPTH")
    ap.add_argument("--consume", choices=("sync", "report"), default=None)
    ap.add_argument("--input", choices=("f32", "u16", "view"), default="f32")
    ap.add_argument("--cam", default=None, metavar="WxH")
    ap.add_argument("--step", type=int, default=2, metavar="K")
    ap.add_argument("--host-reduce", action="store_true")
    ap.add_argument("--unit", type=float, default=None, metavar="MM")
    ap.add_argument("--in-place", action="store_true")
    ap.add_argument("--seeds", choices=("shared", "distinct"), default="shared")
    ap.add_argument("--group", type=int, default=0, metavar="N")
    ap.add_argument("--clean", action="store_true")
    a = ap.parse_args()
    if a.clean and (not a.live or a.drop or a.input not in ("u16", "view")):
        ap.error("--clean cleans a live batch's 16-bit frames: --live --input u16|view, no --drop")
    if a.group < 0 or any(int(x) % max(a.group, 1) for x in a.lanes.split(",")):
        ap.error("--group N: N >= 1 divides every lane count")
    if a.group and (a.hands != "shared" or a.drop):
        ap.error("--group needs --hands shared and no --drop")
    quantised = a.input in ("u16", "view") or a.unit is not None
    cam_mode = a.input == "view" or a.host_reduce
    if a.host_reduce and a.input != "u16":
        ap.error("--host-reduce reduces camera frames for the plain u16 batch: --input u16")
    if (a.cam is not None) != cam_mode and not (a.input == "view" and a.cam is None):
        ap.error("--cam goes with --input view or --host-reduce")
    if cam_mode and a.hands != "shared":
        ap.error("camera frames need --hands shared")
    if (quantised or a.in_place) and (not a.live or a.drop):
        ap.error("--input, --unit and --in-place need --live without --drop")
    if a.in_place and a.hands != "shared":
        ap.error("--in-place needs --hands shared")
    if a.unit is not None and not (np.isfinite(a.unit) and a.unit > 0):
        ap.error("--unit MM: finite and > 0")
    unit = np.float32(1.0 if a.unit is None else a.unit)
    # (no keyword to the begin unless asked for: an older build under A/B lacks them)
    begin_kw = {"input": "u16", "unit_mm": float(unit)} if a.input == "u16" else None
    view = reduce = None
    if cam_mode:
        from hpe.view import View
        W, H = (int(x) for x in (a.cam or "640x480").lower().split("x"))
        K = a.step
        if not 1 <= K <= 8 or 320 * K > W or 240 * K > H:
            ap.error("--cam WxH --step K: the model image enlarged K times must fit the camera's")
        view = View(W, H, W, (H - 240 * K) // 2, (W - 320 * K) // 2, K).check()
        if a.input == "view":
            begin_kw = {"input": "view", "views": view, "unit_mm": float(unit)}
        else:  # the copy an application makes today
            def reduce(cam):
                return cam[view.row0:view.row0 + 240 * K:K, view.col0:view.col0 + 320 * K:K]
    if (a.report or a.consume) and (not a.live or a.drop):
        ap.error("--report and --consume need --live without --drop: reports are the live batch's")
    if a.consume == "report" and not a.report:
        ap.error("--consume report needs --report DEPTH")
    if (a.pacing != "lockstep" or a.drop) and not a.live:
        ap.error("--pacing and --drop need --live: pacing is the live batch's")
    if a.drop < 0 or a.drop == 1:
        ap.error("--drop K: one frame in K per lane, K >= 2 (0: none)")
    if a.raw and a.live:
        ap.error("--raw and --live are two modes")
    if a.window != "off" and not (a.raw or a.live):
        ap.error("--window needs --raw or --live: prepared slots have no preparation to window")
    import torch
    torch.cuda.is_available()
    import hpe
    from hpe import synth
    counts = [int(x) for x in a.lanes.split(",")]
    n = a.frames
    hand = hpe.reference_hand(device=0)
    ctx = hand.ctx
    ub, lb, sd = hpe.reference_bounds()
    pso = hpe.PSO()
    pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, G + 1, 1e-8, 1e-8)
    pso._push(ctx)
    ctx.set_batch_form(a.form)
    if a.pacing != "lockstep":  # (the default is not set: an older build under A/B lacks the call)
        ctx.set_batch_pacing(a.pacing)
    if a.report:  # (likewise)
        ctx.set_batch_report(a.report)
    nb = min(3, max(counts))  # lanes of the check
    yard = wave_yardstick_context(hpe, pso, ctx.batch_wave_wpp(P, nb)) if a.form == "wave" else None
    alone = yard.ctx if yard else None
    if a.live:
        host = make_host_lanes(ctx, max(counts), n)
        feed = host
        if quantised:  # once: the u16 frames, and the floats they stand for
            q16 = [[np.ascontiguousarray(np.rint(f / unit).clip(0, 65535).astype(np.uint16))
                    for f in fr] for fr in host]
            host = [[hpe.depth_u16_to_mm(q, unit) for q in fr] for fr in q16]
            feed = q16 if a.input == "u16" else host
        if cam_mode:  # the camera frames: every model pixel's K x K block holds its value
            def camera(q):
                cam = np.zeros((view.height, view.pitch), np.uint16)
                cam[view.row0:view.row0 + 240 * K, view.col0:view.col0 + 320 * K] = \
                    np.repeat(np.repeat(q, K, axis=0), K, axis=1)
                return cam
            feed = [[camera(q) for q in fr] for fr in q16]
            for b in range(nb):  # the mirror gives the quantised frames back
                for f in range(6):
                    if not np.array_equal(view.reduce(feed[b][f]), q16[b][f]):
                        raise AssertionError("View.reduce of a camera frame is not the frame it was made of")
        check_live_against_alone(ctx, torch, hpe.X0, host[:nb], alone=alone, feed=feed[:nb],
                                 begin_kw=begin_kw, in_place=a.in_place, reduce=reduce)
    elif a.raw:
        raws = make_raw_lanes(ctx, torch, max(counts), n)
        check_raw_against_alone(ctx, torch, hpe.X0, raws[:nb], alone=alone)
    else:
        make_lanes(ctx, max(counts), n)
        if alone:
            make_lanes(alone, nb, n)
        check_against_alone(ctx, torch, hpe.X0, nb, n, alone=alone)
    if alone:
        alone.close()
    for B in counts:
        of = [b // a.group if a.group else b for b in range(B)]  # lane b's stream
        slots = [of[b] * n for b in range(B)]
        if a.hands == "distinct":
            # lane b's own hand: its frames rendered by, and its yardstick run on, a context
            # created with it (in the wave form where this line's check needs that)
            scales = [lane_scale(b, B) for b in range(B)]
            checked = a.form != "wave" or B == counts[0]
            if a.form == "wave" and checked:
                own = [wave_yardstick_context(hpe, pso, ctx.batch_wave_wpp(P, B), s) for s in scales]
            else:
                own = [hpe.scaled_hand(s) for s in scales]
                for h in own:
                    pso._push(h.ctx)
            render = [h.ctx for h in own]
            ctx.set_batch_hands(own)
            if a.live:
                host = [[np.ascontiguousarray(render[b].render_depth(th), dtype=np.float32)
                         for th in synth.trajectory(n, b, revert=0.02)] for b in range(B)]
                feed = host  # the timed runs feed the lanes' own frames too
                if quantised:  # ... quantised as the shared ones above
                    q16 = [[np.ascontiguousarray(np.rint(f / unit).clip(0, 65535).astype(np.uint16))
                            for f in fr] for fr in host]
                    host = [[hpe.depth_u16_to_mm(q, unit) for q in fr] for fr in q16]
                    feed = q16 if a.input == "u16" else host
                if checked:
                    check_live_against_alone(ctx, torch, hpe.X0, host, alone=render, feed=feed,
                                             begin_kw=begin_kw)
            elif a.raw:
                raws = make_raw_lanes(ctx, torch, B, n, render)
                if checked:
                    check_raw_against_alone(ctx, torch, hpe.X0, raws, alone=render)
            else:
                make_lanes(ctx, B, n, render)
                if checked:
                    for b in range(B):  # the lane's first 6 frames in its own context's slots
                        for f in range(6):
                            render[b].prepare_frame(b * n + f, np.ascontiguousarray(
                                render[b].render_depth(synth.trajectory(n, b, revert=0.02)[f])))
                    check_against_alone(ctx, torch, hpe.X0, B, n, alone=render)
            for h in own:
                h.ctx.close()
        if a.raw:
            ptrs = [raws[of[b]].data_ptr() for b in range(B)]

        hist = torch.empty((B, n, 27), dtype=torch.float64, device="cuda:0") if a.raw else None

        tracked = [B * n]
        consumed = [0]
        subs = {k: torch.zeros((k, 27), dtype=torch.float64, device="cuda:0")
                for k in range(1, B + 1)} if a.drop and a.pacing == "lockstep" else None

        def run():
            if a.live and a.drop and a.pacing == "free":
                tracked[0] = run_live_paced(ctx, st, host[:B], n, a.drop)
            elif a.live and a.drop:
                tracked[0] = run_live_rebegin(ctx, torch, st, subs, host[:B], n, a.drop)
            elif a.live:
                consumed[0] = run_live(ctx, st, [feed[of[b]] for b in range(B)], n, a.consume,
                                       begin_kw, a.in_place, reduce)
            elif a.raw:
                ctx.track_raw_batch(P, 1, st.data_ptr(), ptrs, n, frames_per_graph=FPG,
                                    d_hist_ptr=hist.data_ptr())
            else:
                ctx.track_batch(P, 1, st.data_ptr(), slots, n, FPG)
            ctx.check(ctx.lib.hpe_sync(ctx.h))

        st = start_states(torch, hpe.X0, B)
        x0 = st.clone()

        def results():
            return (hist if a.raw else st).cpu().numpy().copy()

        if a.seeds == "distinct":  # (not called otherwise: an older build under A/B lacks it)
            ctx.set_batch_seeds([1000 + b for b in range(B)])
        if a.group:
            ctx.set_batch_groups([a.group] * (B // a.group))
        if a.clean:  # after the check, which runs the lanes uncleaned
            ctx.set_batch_clean([hpe.clean.defaults(float(unit))] * B)
        off = None
        if a.window != "off":  # the same lanes without windows, then the windows for B lanes
            run()
            off = results()
            if a.window == "fixed":
                ctx.set_batch_window("fixed", [hpe.window.WHOLE] * B)
            else:
                w0 = [ctx.lane_window_from_pose(b, hpe.X0, margin_xy=WIN_MARGIN, margin_z=WIN_MARGIN)
                      for b in range(B)]  # (the context's hand in every lane unless --hands distinct)
                ctx.set_batch_window("follow", w0, WIN_MARGIN, WIN_MARGIN)
        times = []
        for rep in range(a.reps + 1):  # the first call captures the graphs
            st.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            times.append(time.perf_counter() - t0)
        el = float(np.median(times[1:]))
        line = {"lanes": B, "frames_per_lane": n, "reps": a.reps,
                "aggregate_tracked_fps": tracked[0] / el,
                "ms_per_batched_frame": el / n * 1e3,
                "workload": "256 p x 30 gen, refine on, N = 250, "
                            + ("host frames, one per lane and call, read from pinned buffers in "
                               "the refine launch, one graph per frame" if a.live else
                               "resident " + ("raw frames prepared in the refine launch" if a.raw
                                              else "prepared frames") + ", 8 frames per graph")
                            + ", one context, seeds 0..B-1"}
        if a.live:
            line["mode"] = "live"
            line["pacing"] = a.pacing
            line["input"] = a.input
            if quantised:
                line["unit_mm"] = float(unit)
            line["in_place"] = a.in_place
            line["host_bytes_copied_per_call"] = 0 if a.in_place else \
                B * (view.pitch * view.height * 2 if a.input == "view" else
                     240 * 320 * (2 if a.input == "u16" else 4))
            if cam_mode:
                line["cam"] = "%dx%d" % (view.width, view.height)
                line["step"] = view.step
                line["host_reduce"] = a.host_reduce
        if a.clean:
            line["clean"] = True
        if a.report:
            line["report_depth"] = a.report
        if a.consume:
            line["consume"] = a.consume
            line["results_consumed"] = consumed[0]
        if a.drop:
            line["drop"] = a.drop
            line["tracked_frames"] = tracked[0]
            line["lane_set_changes"] = "idle lanes" if a.pacing == "free" else "end and begin again"
        if a.form == "wave":
            line["form"] = "wave"
            line["wpp"] = ctx.batch_wave_wpp(P, B)
        if a.raw:
            line["mode"] = "raw"
        if a.raw or a.live:
            line["window"] = a.window
        if a.hands == "distinct":
            line["hands"] = "distinct"
            line["hand_scales"] = [round(s, 6) for s in scales]
            line["checked_against_own_hand_contexts"] = checked
        if a.seeds == "distinct":
            line["seeds"] = "distinct"
        if a.group:
            line["group"] = a.group
            line["final_cost"] = [float(v) for v in st.cpu().numpy()[:, 26]]
        if off is not None:
            line["equals_off"] = bool(np.array_equal(results(), off))
        # the timed run's results (raw: the histories; else the final states), for an A/B of builds
        line["results_sha1"] = hashlib.sha1(results().tobytes()).hexdigest()[:16]
        if a.profile:
            st.copy_(x0)
            torch.cuda.synchronize()
            line["kernels"] = kernel_means_us(ctx, run)
        print(json.dumps(line), flush=True)
        if a.window != "off":
            ctx.set_batch_window("off")
        if a.hands == "distinct":
            ctx.set_batch_hands(None)
        if a.seeds == "distinct":
            ctx.set_batch_seeds(None)
        if a.group:
            ctx.set_batch_groups(None)
        if a.clean:
            ctx.set_batch_clean(None)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
