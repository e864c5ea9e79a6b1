"""hpe -- Python host mirror of the reference's PSO / costfunc / handmodel API.

Same class and method names, argument meaning and in-place (non-const reference)
semantics as /root/reference/src/{handmodel,observedmodel,costfunc,PSO}.h, over the
C ABI of include/hpe.h (libhpe.so: gfx950 HIP kernels).  numpy arrays stand in for
Armadillo vec/mat/uvec: a 26-vector theta, a (48, 3) sphere matrix, an int32 matchId.
Every compute call runs on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path

import numpy as np

from . import _lib, clean, group, locate, report, view, window
from ._lib import HpeError, ptr

__all__ = ["handmodel", "observedmodel", "costfunc", "PSO", "reference_hand", "scaled_hand",
           "HpeError",
           "gnd_truth_err",
           "Context", "preprocess_depth", "reference_bounds", "X0", "depth_u16_to_mm"]

IMG_H, IMG_W = 240, 320
# testmodel.cpp:34-40
TB_SPHERES = (2, 2, 2, 2)
FG_SPHERES = (4, 2, 2, 2)
SPACING = (-1.86, -1.86, 0.0, 1.91, 3.84)
CMC = (150.0, 107.5, 89.8, 76.5, 59.6)
X0 = np.array([0, -10, -40, 0, 3, 32, 6, 9, 8, 9, 3, 9, 9, 6, 1, 9, 8, 7, 4, 8, 7, 6, 2,
               7, 7, 7], dtype=np.float64)


def reference_bounds():
    """ub, lb, std of testmodel.cpp:74-98."""
    ub = np.zeros(26); lb = np.zeros(26); sd = np.zeros(26)
    ub[0:3], ub[3:6], lb[0:3], lb[3:6] = 180, 100, -180, -100
    for k in range(5):
        ub[6 + 4 * k:10 + 4 * k] = (15, 90, 110, 90)
        lb[6 + 4 * k:10 + 4 * k] = (-15, 0, 0, 0)
    sd[0:3], sd[3:6], sd[6:26] = 9.0, 7.0, 9.0
    return ub, lb, sd


# a live batch's frame formats ("view": uint16 camera frames read through lane views)
BATCH_INPUTS = {"f32": np.float32, "u16": np.uint16, "view": np.uint16}


def depth_u16_to_mm(frame_u16, unit_mm=1.0):
    """The float mm frame a 16-bit depth frame stands for in a u16 live batch
    (hpe_batch_pipeline_begin_u16): float32(u) * float32(unit_mm), one fp32 multiply per pixel,
    0 stays 0.  frame_u16 must be a uint16 array (nothing is converted silently)."""
    f = np.asarray(frame_u16)
    if f.dtype != np.uint16:
        raise TypeError(f"depth_u16_to_mm takes uint16 frames, got {f.dtype}")
    return f.astype(np.float32) * np.float32(unit_mm)


BATCH_FORMS = {"auto": _lib.BATCH_FORM_AUTO, "wave": _lib.BATCH_FORM_WAVE}
BATCH_PACINGS = {"lockstep": _lib.PACING_LOCKSTEP, "free": _lib.PACING_FREE}
WINDOW_MODES = {"off": _lib.WINDOW_OFF, "fixed": _lib.WINDOW_FIXED, "follow": _lib.WINDOW_FOLLOW}


def _check(lib, ctx, rc):
    if rc != 0:
        msg = lib.hpe_last_error(ctx).decode() if ctx else ""
        raise HpeError(f"hpe error {rc}: {msg}")


class Context:
    """One hpe_ctx: device buffers, the hand constants and one HIP stream."""

    def __init__(self, params: _lib.HandParams, device: int = 0):
        self.lib = _lib.load()
        self._h = C.c_void_p()
        rc = self.lib.hpe_create(C.byref(self._h), device, C.byref(params))
        if rc != 0:
            raise HpeError(f"hpe_create failed ({rc}): no gfx950 device {device}?")
        self.device = device
        self.frame_token = None

    @property
    def h(self):
        return self._h

    def check(self, rc):
        _check(self.lib, self._h, rc)

    def close(self):
        if self._h:
            self.lib.hpe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- frames
    @property
    def refine_exact(self) -> bool:
        """True: refine_init_pose places spheres by the reference's DH chain on every
        evaluation; False (default): the hand-frame form (hpe_set_refine_exact).

        The two forms differ in fp64 operation order only (centres within 1e-12 cm).  Over
        the 400-frame sequence test the default form's refine took a different number of
        evaluations than the reference-order oracle on 6 frames, each a replayed near-tie
        (relative margin < 1e-13), and the tracked poses stayed within 2.2e-7 per frame and
        2.8e-7 of the free-running reference-order oracle."""
        return bool(self.lib.hpe_get_refine_exact(self.h))

    @refine_exact.setter
    def refine_exact(self, exact: bool):
        self.check(self.lib.hpe_set_refine_exact(self.h, 1 if exact else 0))

    @property
    def refine_spec(self) -> bool:
        """True (default): the refine launch of clouds of at most 2048 points carries a second
        workgroup that runs the translation block ahead of a failing rotation search
        (hpe_set_refine_spec); False: the one-workgroup form.  The results are the same bit
        for bit."""
        return bool(self.lib.hpe_get_refine_spec(self.h))

    @refine_spec.setter
    def refine_spec(self, on: bool):
        self.check(self.lib.hpe_set_refine_spec(self.h, 1 if on else 0))

    def store_frame(self, slot, depth_cm, dt, cloud, scale, dtmax, K):
        depth_cm = np.ascontiguousarray(depth_cm, dtype=np.float64)
        dt = np.ascontiguousarray(dt, dtype=np.float32)
        cloud = np.ascontiguousarray(cloud, dtype=np.float64).reshape(-1, 3)
        f = _lib.Frame(ptr(depth_cm, C.c_double), ptr(dt, C.c_float), ptr(cloud, C.c_double),
                       len(cloud), float(scale), float(dtmax),
                       (C.c_double * 9)(*np.asarray(K, dtype=np.float64).ravel()))
        self.check(self.lib.hpe_store_frame(self._h, slot, C.byref(f)))

    def select_frame(self, slot):
        self.check(self.lib.hpe_select_frame(self._h, slot))

    def prepare_frame(self, slot, depth_mm, to_cm=True, downsample=True, focal=241.42):
        """observedmodel::next_frame on the GPU into `slot` (asynchronous)."""
        d = np.ascontiguousarray(depth_mm, dtype=np.float32).reshape(IMG_H, IMG_W)
        self.check(self.lib.hpe_prepare_frame(self._h, slot, ptr(d, C.c_float), int(to_cm),
                                              int(downsample), float(focal)))

    def pipeline_begin(self, depth_mm, to_cm=True, downsample=True, focal=241.42):
        d = np.ascontiguousarray(depth_mm, dtype=np.float32).reshape(IMG_H, IMG_W)
        self.check(self.lib.hpe_pipeline_begin(self._h, ptr(d, C.c_float), int(to_cm),
                                               int(downsample), float(focal)))

    def track_pipelined(self, num_p, refine, d_state_ptr, next_depth_mm=None):
        """Track the pipeline's current frame into the 27 device doubles at d_state_ptr and
        prepare next_depth_mm (host) as the following frame."""
        nd = None
        if next_depth_mm is not None:
            nd = np.ascontiguousarray(next_depth_mm, dtype=np.float32).reshape(IMG_H, IMG_W)
        self.check(self.lib.hpe_track_pipelined(self._h, int(num_p), int(refine),
                                                C.c_void_p(d_state_ptr),
                                                ptr(nd, C.c_float) if nd is not None else None))

    def track_sequence(self, num_p, refine, d_state_ptr, first_slot, n, frames_per_graph=0,
                       d_hist_ptr=None):
        """Track resident frames first_slot .. first_slot+n-1 in order (test_full's loop),
        frames_per_graph of them per graph launch; frame f's {bestp, cost} to d_hist_ptr +
        27 f (device, optional).  Asynchronous on the context stream."""
        self.check(self.lib.hpe_track_sequence_dev(
            self._h, int(num_p), int(refine), C.c_void_p(d_state_ptr), int(first_slot), int(n),
            int(frames_per_graph), C.c_void_p(d_hist_ptr) if d_hist_ptr else None))

    def track_batch(self, num_p, refine, d_states_ptr, first_slots, n, frames_per_graph=0,
                    d_hist_ptr=None):
        """Track B = len(first_slots) independent sequences in the same launches: lane b is
        track_sequence(num_p, refine, d_states_ptr + 27*8 b, first_slots[b], n, ...) bit for
        bit, with its history at d_hist_ptr + 27*8 n b (device, optional).  d_states_ptr:
        B x 27 device doubles.  Asynchronous on the context stream."""
        fs = [int(s) for s in first_slots]
        if not 1 <= len(fs) <= _lib.BATCH_MAX:
            raise ValueError(f"track_batch takes 1..{_lib.BATCH_MAX} lanes, got {len(fs)}")
        if not d_states_ptr:
            raise ValueError("track_batch needs the device states")
        arr = (C.c_int32 * len(fs))(*fs)
        self.check(self.lib.hpe_track_batch_dev(
            self._h, int(num_p), int(refine), len(fs), C.c_void_p(d_states_ptr), arr, int(n),
            int(frames_per_graph), C.c_void_p(d_hist_ptr) if d_hist_ptr else None))

    def track_raw_sequence(self, num_p, refine, d_state_ptr, d_raw_ptr, n, to_cm=True,
                           downsample=True, focal=241.42, frames_per_graph=0, d_hist_ptr=None):
        """Track n raw depth frames resident in HBM (d_raw_ptr: n x 240x320 float mm) in
        order (test_full's loop), each next frame prepared inside the previous frame's
        refine launch, frames_per_graph per graph launch; frame f's {bestp, cost} to
        d_hist_ptr + 27 f (device, optional).  Asynchronous on the context stream."""
        self.check(self.lib.hpe_track_raw_sequence_dev(
            self._h, int(num_p), int(refine), C.c_void_p(d_state_ptr), C.c_void_p(d_raw_ptr),
            int(n), int(to_cm), int(downsample), float(focal), int(frames_per_graph),
            C.c_void_p(d_hist_ptr) if d_hist_ptr else None))

    def track_raw_batch(self, num_p, refine, d_states_ptr, d_raw_ptrs, n, to_cm=True,
                        downsample=True, focal=241.42, frames_per_graph=0, d_hist_ptr=None):
        """Track B = len(d_raw_ptrs) resident raw sequences in the same launches: lane b is
        track_raw_sequence(num_p, refine, d_states_ptr + 27*8 b, d_raw_ptrs[b], n, ...) bit for
        bit, with its history at d_hist_ptr + 27*8 n b (device, optional).  d_raw_ptrs: device
        pointers, each to n x 240x320 float mm (lanes may share one).  d_states_ptr: B x 27
        device doubles.  Asynchronous on the context stream."""
        rp = [int(p) for p in d_raw_ptrs]
        if not 1 <= len(rp) <= _lib.BATCH_MAX:
            raise ValueError(f"track_raw_batch takes 1..{_lib.BATCH_MAX} lanes, got {len(rp)}")
        if not d_states_ptr:
            raise ValueError("track_raw_batch needs the device states")
        arr = (C.c_void_p * len(rp))(*rp)
        self.check(self.lib.hpe_track_raw_batch_dev(
            self._h, int(num_p), int(refine), len(rp), C.c_void_p(d_states_ptr), arr, int(n),
            int(to_cm), int(downsample), float(focal), int(frames_per_graph),
            C.c_void_p(d_hist_ptr) if d_hist_ptr else None))

    def _host_frames(self, what, depths, dtype=np.float32, views=None):
        """The lanes' host frames as 240x320 arrays of `dtype` (views: lane b's as a
        (height, pitch) camera frame of views[b]) and the array of their addresses
        (the arrays must outlive the call that takes the addresses).  Under the "free" pacing
        (set_batch_pacing) an entry may be None: a null address, no frame for that lane.
        float32 frames are converted from whatever is given; uint16 frames must be uint16
        already.  An array that is contiguous and of the dtype is never copied, so a
        batch_frame_buffer view reaches the library with the buffer's own address."""
        ds = list(depths)
        if not 1 <= len(ds) <= _lib.BATCH_MAX:
            raise ValueError(f"{what} takes 1..{_lib.BATCH_MAX} lanes, got {len(ds)}")
        free = getattr(self, "_pacing", _lib.PACING_LOCKSTEP) == _lib.PACING_FREE
        if not free and any(d is None for d in ds):
            raise ValueError(f"{what}: a frame for every lane or for none (lanes advance in "
                             "lockstep)")
        if dtype == np.uint16:
            for d in ds:
                if d is not None and np.asarray(d).dtype != np.uint16:
                    raise TypeError(f"{what}: a u16 batch takes uint16 frames, got "
                                    f"{np.asarray(d).dtype} (nothing is converted silently)")
        elif any(d is not None and np.asarray(d).dtype == np.uint16 for d in ds):
            raise TypeError(f"{what}: a float batch was given uint16 frames (begin the batch "
                            "with input=\"u16\", or convert with depth_u16_to_mm)")
        if views is not None and len(views) != len(ds):
            raise ValueError(f"{what}: {len(ds)} lane frames for {len(views)} views")
        shapes = ([(IMG_H, IMG_W)] * len(ds) if views is None
                  else [(v.height, v.pitch) for v in views])
        for d, sh in zip(ds, shapes):
            if d is not None and np.asarray(d).size != sh[0] * sh[1]:
                raise ValueError(f"{what}: a frame of {np.asarray(d).size} pixels, the lane's is "
                                 f"{sh[0]} x {sh[1]}")
        fr = [None if d is None else
              np.ascontiguousarray(d, dtype=dtype).reshape(sh) for d, sh in zip(ds, shapes)]
        return fr, (C.c_void_p * len(fr))(*[None if f is None else f.ctypes.data for f in fr])

    def batch_pipeline_begin(self, depths, to_cm=True, downsample=True, focal=241.42,
                             input="f32", unit_mm=1.0, views=None):
        """Begin a live batch of B = len(depths) lanes: lane b's first raw frame (host, float
        mm 240x320) is copied and prepared.  Ends a live batch in progress.
        input="u16": the batch's frames are uint16 arrays of unit_mm millimetres per count
        (hpe_batch_pipeline_begin_u16), read as such by the device; lane b then equals the
        float batch on depth_u16_to_mm(frame, unit_mm) bit for bit.  The batch keeps its format:
        track_batch_pipelined follows it.
        input="view": uint16 frames at the camera's own resolution (hpe_batch_pipeline_begin_view),
        lane b's a (height, pitch) frame of views[b] (hpe.view.View or anything as_view takes);
        focal is the model image's, fx / step.  Lane b then equals the float batch on
        depth_u16_to_mm(views[b].reduce(frame), unit_mm) bit for bit."""
        if input not in BATCH_INPUTS:
            raise ValueError(f"batch input {input!r} is not one of {sorted(BATCH_INPUTS)}")
        if (input == "view") != (views is not None):
            raise ValueError("views go with input=\"view\", and input=\"view\" needs views")
        vs = None if views is None else [view.as_view(v).check() for v in views]
        fr, arr = self._host_frames("batch_pipeline_begin", depths, BATCH_INPUTS[input], vs)
        if input == "view":
            tab = (_lib.View * len(vs))(*[_lib.View(*[getattr(v, f) for f in view.FIELDS])
                                          for v in vs])
            self.check(self.lib.hpe_batch_pipeline_begin_view(
                self._h, len(fr), arr, tab, float(unit_mm), int(to_cm), int(downsample),
                float(focal)))
        elif input == "u16":
            self.check(self.lib.hpe_batch_pipeline_begin_u16(
                self._h, len(fr), arr, float(unit_mm), int(to_cm), int(downsample), float(focal)))
        else:
            self.check(self.lib.hpe_batch_pipeline_begin(self._h, len(fr), arr, int(to_cm),
                                                         int(downsample), float(focal)))
        self._live_lanes = len(fr)
        self._live_input = input
        self._live_views = vs

    def batch_frame_buffer(self, lane):
        """Lane `lane`'s pinned buffer that the next track_batch_pipelined reads, as a 240x320
        numpy view (float32 or uint16, the batch's format; for a view batch the lane's
        (height, pitch) uint16 camera frame) over the library's memory
        (hpe_batch_frame_buffer: it first waits until the device has read the frame the buffer
        last held).  Write the lane's next frame into it and pass the view back as that lane's
        entry of next_depths: nothing is copied for the lane.  Ask again after every call: the
        view of an earlier call is refused (HPE_E_ARG, "stale frame buffer")."""
        buf, n = C.c_void_p(), C.c_size_t(0)
        self.check(self.lib.hpe_batch_frame_buffer(self._h, int(lane), C.byref(buf), C.byref(n)))
        dt = BATCH_INPUTS[getattr(self, "_live_input", "f32")]
        raw = (C.c_char * n.value).from_address(buf.value)
        vs = getattr(self, "_live_views", None)
        if vs is not None and 0 <= int(lane) < len(vs):
            return np.frombuffer(raw, dtype=dt).reshape(vs[int(lane)].height, vs[int(lane)].pitch)
        return np.frombuffer(raw, dtype=dt).reshape(IMG_H, IMG_W)

    def track_batch_pipelined(self, num_p, refine, d_states_ptr, next_depths=None):
        """Track the current frame of every lane of the live batch in the same launches -- lane b
        is track_pipelined(num_p, refine, d_states_ptr + 27*8 b, next_depths[b]) bit for bit --
        and prepare next_depths (one host frame per lane, copied before return) as the following
        frames; None ends the batch.  d_states_ptr: B x 27 device doubles.  Asynchronous on the
        context stream.  The frames are of the begin's format (uint16 arrays for a u16 batch); an
        entry that is the lane's batch_frame_buffer view was filled in place and is not copied."""
        if not d_states_ptr:
            raise ValueError("track_batch_pipelined needs the device states")
        inp = getattr(self, "_live_input", "f32")  # the begin's format
        if next_depths is None:
            # the lane count of the begin (1 without one: the library then reports the state)
            B, arr = getattr(self, "_live_lanes", 0) or 1, None
        else:
            fr, arr = self._host_frames("track_batch_pipelined", next_depths, BATCH_INPUTS[inp],
                                        getattr(self, "_live_views", None))
            B = len(fr)
        track = (self.lib.hpe_track_batch_pipelined_u16 if inp in ("u16", "view")
                 else self.lib.hpe_track_batch_pipelined)
        self.check(track(self._h, int(num_p), int(refine), B, C.c_void_p(d_states_ptr), arr))

    def set_batch_pacing(self, pacing):
        """Whether the lanes of a live batch advance in lockstep (hpe_set_batch_pacing), read at
        batch_pipeline_begin: "lockstep" / 0 (default: a frame for every lane or for none) or
        "free" / 1 -- batch_pipeline_begin and track_batch_pipelined then accept None entries: a
        lane given no frame idles for that call, bit for bit untouched, and a lane may start empty
        and join later; a lane tracks in a call iff it holds a prepared frame (batch_pending).
        A live batch in progress keeps its pacing: a different one raises (HPE_E_STATE)."""
        if isinstance(pacing, str):
            if pacing not in BATCH_PACINGS:
                raise ValueError(f"batch pacing {pacing!r} is not one of {sorted(BATCH_PACINGS)}")
            pacing = BATCH_PACINGS[pacing]
        self.check(self.lib.hpe_set_batch_pacing(self._h, int(pacing)))
        self._pacing = int(pacing)

    def batch_pending(self) -> int:
        """Bit b set: lane b of the live batch holds a prepared frame that the next
        track_batch_pipelined tracks (hpe_batch_pending; host bookkeeping, no synchronisation)."""
        m = C.c_uint32(0)
        self.check(self.lib.hpe_batch_pending(self._h, C.byref(m)))
        return m.value

    def set_batch_report(self, depth, watch=None):
        """Lane reports (hpe_set_batch_report), read at batch_pipeline_begin: depth 0 (default)
        is off; 2..64 gives every lane a ring of `depth` reports in pinned host memory, written
        by the device inside every tracked frame's graph -- the lane's state row, its 21 joints
        under the lane's hand, their pixels (hpe.report.project_joints), n and health flags.
        watch: None, or (cost_max, n_min, streak) / hpe._lib.ReportWatch -- a tracked frame is
        SUSPECT iff not cost <= cost_max or n < n_min, the lane LOST after `streak` in a row.
        A live batch in progress keeps its setting: a different one raises (HPE_E_STATE)."""
        if watch is not None and not isinstance(watch, _lib.ReportWatch):
            cost_max, n_min, streak = watch
            watch = _lib.ReportWatch(float(cost_max), int(n_min), int(streak))
        self.check(self.lib.hpe_set_batch_report(self._h, int(depth),
                                                 C.byref(watch) if watch is not None else None))

    def batch_report(self, lane, seq=0, raw=False):
        """Lane `lane`'s report number seq, or its newest complete one (seq = 0; .seq == 0: none
        yet), as hpe.report.Report (raw: the hpe._lib.LaneReport).  Never blocks, never touches
        the stream (hpe_batch_report); a seq not in the ring raises (HPE_E_STATE)."""
        r = _lib.LaneReport()
        self.check(self.lib.hpe_batch_report(self._h, int(lane), int(seq), C.byref(r)))
        return r if raw else report.as_report(r)

    def batch_report_wait(self, lane, seq=0, timeout_ms=2000, raw=False):
        """Wait, at most timeout_ms, for lane `lane`'s report seq to complete (seq = 0: the last
        one enqueued for the lane) and return it (hpe_batch_report_wait); no synchronisation of
        the stream.  Raises on expiry (HPE_E_HIP)."""
        r = _lib.LaneReport()
        self.check(self.lib.hpe_batch_report_wait(self._h, int(lane), int(seq), int(timeout_ms),
                                                  C.byref(r)))
        return r if raw else report.as_report(r)

    def batch_lost(self) -> int:
        """Bit b set: lane b's newest report has HPE_REPORT_F_LOST (hpe_batch_lost); the
        application re-initialises such a lane with batch_pipeline_optimise."""
        m = C.c_uint32(0)
        self.check(self.lib.hpe_batch_lost(self._h, C.byref(m)))
        return m.value

    def lane_joints(self, B, n, d_hist_ptr, d_joints_ptr, d_px_ptr=None, focal=241.42):
        """The reports' joints and pixels for a resident batch's history (hpe_lane_joints_dev):
        row b n + f of d_hist (27 doubles) under lane b's hand into d_joints [B][n][21][3] and,
        if given, d_px [B][n][21][2] -- device pointers.  Asynchronous on the context stream."""
        self.check(self.lib.hpe_lane_joints_dev(
            self._h, int(B), int(n), C.c_void_p(d_hist_ptr) if d_hist_ptr else None, float(focal),
            C.c_void_p(d_joints_ptr) if d_joints_ptr else None,
            C.c_void_p(d_px_ptr) if d_px_ptr else None))

    def pso_optimise_batch(self, num_p, d_states_ptr, slots, d_trace_ptr=None):
        """pso_optimise of B = len(slots) lanes in the same launches (hpe_pso_optimise_batch):
        lane b is select_frame(slots[b]) + hpe_pso_optimise from x0 = d_states_ptr + 27*8 b, bit
        for bit, on a context created with lane b's hand (set_batch_hands).  d_states_ptr: B x 27
        device doubles {x0 -> bestp, cost}; d_trace_ptr (device, optional): B x (maxiter-1) gbest
        costs.  Asynchronous on the context stream."""
        sl = [int(s) for s in slots]
        if not 1 <= len(sl) <= _lib.BATCH_MAX:
            raise ValueError(f"pso_optimise_batch takes 1..{_lib.BATCH_MAX} lanes, got {len(sl)}")
        if not d_states_ptr:
            raise ValueError("pso_optimise_batch needs the device states")
        arr = (C.c_int32 * len(sl))(*sl)
        self.check(self.lib.hpe_pso_optimise_batch(
            self._h, int(num_p), len(sl), C.c_void_p(d_states_ptr), arr,
            C.c_void_p(d_trace_ptr) if d_trace_ptr else None))

    def batch_pipeline_optimise(self, num_p, d_states_ptr, lanes=None, d_trace_ptr=None):
        """The same on the live batch's current prepared frames, through the lanes' windows and
        hands (hpe_batch_pipeline_optimise).  lanes: bit b set = lane b is optimised, the other
        lanes' rows stay untouched; None: every lane in lockstep, batch_pending() under the "free"
        pacing.  Changes nothing of the live batch itself.  Asynchronous on the context stream."""
        if not d_states_ptr:
            raise ValueError("batch_pipeline_optimise needs the device states")
        B = getattr(self, "_live_lanes", 0) or 1  # (1 without a begin: the library reports it)
        if lanes is None:
            free = getattr(self, "_pacing", _lib.PACING_LOCKSTEP) == _lib.PACING_FREE
            lanes = self.batch_pending() if free else (1 << B) - 1
        self.check(self.lib.hpe_batch_pipeline_optimise(
            self._h, int(num_p), B, C.c_void_p(d_states_ptr), int(lanes),
            C.c_void_p(d_trace_ptr) if d_trace_ptr else None))

    # ---- lane location (hpe_locate_depth, hpe_batch_pipeline_locate)
    @staticmethod
    def _locate_params(params):
        p = locate.as_params(params)
        return _lib.LocateParams(_lib.Window(*p.search), p.bin, p.slab, p.half_xy, p.half_z,
                                 p.skip, p.min_pixels)

    @staticmethod
    def _locate_result(r, raw):
        if raw:
            return r
        return locate.Result(int(r.found), int(r.k_near), int(r.m1), int(r.m2), tuple(r.px),
                             tuple(r.centre), window.as_window(r.window))

    def locate_depth(self, depth, focal=241.42, params=None, to_cm=True, unit_mm=None, raw=False):
        """The location rule on one host frame, on the device (hpe_locate_depth; synchronises):
        float32 mm pixels, or uint16 pixels of unit_mm each.  params: an hpe.locate.Params (None:
        the library's defaults).  Returns an hpe.locate.Result, which equals
        hpe.locate.locate(...) on the same arguments bit for bit (raw: the hpe._lib.Locate)."""
        d = np.asarray(depth)
        u16 = unit_mm is not None
        if u16 != (d.dtype == np.uint16):
            raise TypeError("locate_depth: uint16 frames come with their unit_mm, float frames "
                            "without one (nothing is converted silently)")
        d = np.ascontiguousarray(d, dtype=np.uint16 if u16 else np.float32).reshape(IMG_H, IMG_W)
        lp = self._locate_params(params) if params is not None else None
        r = _lib.Locate()
        self.check(self.lib.hpe_locate_depth(
            self._h, C.c_void_p(d.ctypes.data), int(u16), float(unit_mm) if u16 else 1.0,
            int(to_cm), float(focal), C.byref(lp) if lp is not None else None, C.byref(r)))
        return self._locate_result(r, raw)

    def batch_pipeline_locate(self, d_states_ptr, templates, lanes=None, params=None):
        """Locate the hand of the selected pending lanes of the live batch in their current raw
        frames, on the device and asynchronously (hpe_batch_pipeline_locate): a found lane gets
        its window (the table's current parity; both under "fixed"), its current frame prepared
        again through it, and its row of d_states_ptr = its template (one 26-pose per lane, or
        one for all) moved onto the located centre (hpe.locate.place).  A lane that is not
        found, or not selected, stays untouched.  lanes: bit b = lane b; None: every lane in
        lockstep, batch_pending() under the "free" pacing.  params: None (the defaults), one
        hpe.locate.Params for all lanes, or a list of one per lane."""
        if not d_states_ptr:
            raise ValueError("batch_pipeline_locate needs the device states")
        B = getattr(self, "_live_lanes", 0) or 1  # (1 without a begin: the library reports it)
        if lanes is None:
            free = getattr(self, "_pacing", _lib.PACING_LOCKSTEP) == _lib.PACING_FREE
            lanes = self.batch_pending() if free else (1 << B) - 1
        t = np.asarray(templates, dtype=np.float64)
        t = np.ascontiguousarray(np.broadcast_to(t.reshape(-1, 26) if t.ndim > 1 else t[:26], (B, 26)))
        arr = None
        if params is not None:
            ps = ([params] * B if isinstance(params, locate.Params) else list(params))
            if len(ps) != B:
                raise ValueError(f"batch_pipeline_locate: {len(ps)} parameter sets for {B} lanes")
            arr = (_lib.LocateParams * B)(*[self._locate_params(p) for p in ps])
        self.check(self.lib.hpe_batch_pipeline_locate(
            self._h, B, C.c_void_p(d_states_ptr), int(lanes), ptr(t, C.c_double), arr))

    def batch_locate_result(self, lane, timeout_ms=2000, raw=False):
        """Lane `lane`'s newest locate result (hpe_batch_locate_result): waits, at most
        timeout_ms, for the last locate enqueued for the lane, without synchronising the stream;
        raises on expiry (HPE_E_HIP).  Returns (seq, hpe.locate.Result) -- seq counts the lane's
        locates since the begin, 0: none yet -- or the hpe._lib.Locate with raw."""
        r = _lib.Locate()
        self.check(self.lib.hpe_batch_locate_result(self._h, int(lane), int(timeout_ms), C.byref(r)))
        return r if raw else (int(r.seq), self._locate_result(r, False))

    def set_batch_form(self, form):
        """The form of pso_evolve in track_batch, track_raw_batch and the live batch
        (hpe_set_batch_form): "auto" / 0 (default: a workgroup per particle, num_p in the wave
        form refused) or "wave" / 1 (every lane in the wave-per-particle form, at any num_p; lane
        b is then the single-sequence call on a context created under HPE_PSO_FORM=wave and
        HPE_PSO_WPP=batch_wave_wpp(num_p, B), bit for bit).  A live batch in progress keeps its
        form: a different one raises (HPE_E_STATE)."""
        if isinstance(form, str):
            if form not in BATCH_FORMS:
                raise ValueError(f"batch form {form!r} is not one of {sorted(BATCH_FORMS)}")
            form = BATCH_FORMS[form]
        self.check(self.lib.hpe_set_batch_form(self._h, int(form)))

    def set_batch_window(self, mode, init=None, margin_xy=0.0, margin_z=0.0):
        """Segment every lane's depth by a window (hpe_set_batch_window) in track_raw_batch and
        the live batch, from the next call or begin on: "off" / 0 (default), "fixed" / 1 (lane
        b's every frame masked by init[b]) or "follow" / 2 (frame 0 by init[b], later frames by
        the pose rule on the lane's own tracked pose, hpe.window.from_spheres, with the two
        margins).  init: one window per lane (hpe.window.Window, any 6-sequence or
        hpe._lib.Window); the batch calls then take exactly len(init) lanes.  A live batch in
        progress keeps what it began with: the call raises (HPE_E_STATE)."""
        if isinstance(mode, str):
            if mode not in WINDOW_MODES:
                raise ValueError(f"window mode {mode!r} is not one of {sorted(WINDOW_MODES)}")
            mode = WINDOW_MODES[mode]
        if init is None:
            B, arr = 1, None
        else:
            ws = [window.as_window(w) for w in init]
            B = len(ws)
            arr = (_lib.Window * max(B, 1))(*[_lib.Window(*w) for w in ws])
        self.check(self.lib.hpe_set_batch_window(self._h, int(mode), B, arr, float(margin_xy),
                                                 float(margin_z)))

    def window_from_pose(self, theta, focal=241.42, margin_xy=0.0, margin_z=0.0):
        """The pose rule on the device (hpe_window_from_pose): the window of the context hand at
        pose theta, as FOLLOW computes it.  Synchronises."""
        th = _lib.as_f64(theta, (26,))
        w = _lib.Window()
        self.check(self.lib.hpe_window_from_pose(self._h, ptr(th, C.c_double), float(focal),
                                                 float(margin_xy), float(margin_z), C.byref(w)))
        return window.as_window(w)

    def set_batch_hands(self, hands):
        """A hand model per lane (hpe_set_batch_hands) in track_batch, track_raw_batch and the
        live batch, from the next call or begin on: hands is a list of handmodel or
        hpe._lib.HandParams, one per lane -- lane b is then the single-sequence call on a context
        created with hands[b], bit for bit -- and the batch calls take exactly len(hands) lanes;
        None (default): every lane tracks with the context's hand.  The single-sequence calls
        always use the context's hand.  A live batch in progress keeps the hands it began with:
        the call raises (HPE_E_STATE)."""
        if hands is None:
            self.check(self.lib.hpe_set_batch_hands(self._h, 0, None))
            return
        ps = [getattr(h, "params", h) for h in hands]
        if any(not isinstance(p, _lib.HandParams) for p in ps):
            raise TypeError("set_batch_hands takes handmodel or HandParams entries")
        arr = (_lib.HandParams * max(len(ps), 1))(*ps)
        self.check(self.lib.hpe_set_batch_hands(self._h, len(ps), arr))

    def set_batch_seeds(self, seeds):
        """A seed per lane (hpe_set_batch_seeds) in track_batch, track_raw_batch and the live
        batch, from the next call or begin on: lane b's pso_evolve draws under seeds[b] -- it is
        then the single-sequence call on a context after set_seed(seeds[b]), bit for bit -- and
        the batch calls take exactly len(seeds) lanes; None (default): every lane draws under the
        context's seed.  The batch optimiser keeps the context's seed.  A live batch in progress
        keeps the seeds it began with: the call raises (HPE_E_STATE)."""
        if seeds is None:
            self.check(self.lib.hpe_set_batch_seeds(self._h, 0, None))
            return
        s = [int(v) for v in seeds]
        arr = (C.c_uint64 * max(len(s), 1))(*s)
        self.check(self.lib.hpe_set_batch_seeds(self._h, len(s), arr))

    def set_batch_groups(self, sizes):
        """Lane groups (hpe_set_batch_groups): sizes lists the groups' lane counts, consecutive
        lanes, summing to the batch's B; after every tracked frame each group's rows of d_states
        (and of d_hist) become the group's best own row by hpe.group.pick's rule, and the lanes'
        own rows are kept for batch_group_rows.  None or an empty list (default): no groups."""
        if sizes is None or len(sizes) == 0:
            self.check(self.lib.hpe_set_batch_groups(self._h, 0, 0, None))
            return
        z = [int(v) for v in sizes]
        arr = (C.c_int32 * len(z))(*z)
        self.check(self.lib.hpe_set_batch_groups(self._h, sum(z), len(z), arr))

    def batch_group_pick(self, d_states_ptr, B):
        """The groups' pick on the B x 27 device rows at d_states_ptr (hpe_batch_group_pick),
        asynchronous on the context stream: every group's rows become the group's best row."""
        self.check(self.lib.hpe_batch_group_pick(self._h, int(B), C.c_void_p(int(d_states_ptr))))

    def batch_group_rows(self, B):
        """Every lane's own {bestp, cost} of the last grouped frame it tracked, (B, 27)
        (hpe_batch_group_rows).  Synchronises."""
        rows = np.zeros((int(B), 27))
        self.check(self.lib.hpe_batch_group_rows(self._h, int(B), ptr(rows, C.c_double)))
        return rows

    def lane_window_from_pose(self, lane, theta, focal=241.42, margin_xy=0.0, margin_z=0.0):
        """window_from_pose under lane `lane`'s hand (hpe_lane_window_from_pose): init[lane] of a
        "follow" batch with lane hands.  Synchronises."""
        th = _lib.as_f64(theta, (26,))
        w = _lib.Window()
        self.check(self.lib.hpe_lane_window_from_pose(self._h, int(lane), ptr(th, C.c_double),
                                                      float(focal), float(margin_xy),
                                                      float(margin_z), C.byref(w)))
        return window.as_window(w)

    def batch_windows_readback(self, parity, B):
        """The B lane windows of one buffer parity (frame f of a call is prepared into parity
        f & 1), as a list of hpe.window.Window.  Synchronises."""
        arr = (_lib.Window * max(int(B), 1))()
        self.check(self.lib.hpe_batch_windows_readback(self._h, int(parity), int(B), arr))
        return [window.as_window(arr[b]) for b in range(int(B))]

    def batch_views_readback(self, B):
        """The lane views the device table holds (hpe_batch_views_readback; synchronises): B
        hpe.view.View of the last view batch begun."""
        out = (_lib.View * int(B))()
        self.check(self.lib.hpe_batch_views_readback(self._h, int(B), out))
        return [view.as_view(v) for v in out]

    @staticmethod
    def _clean_par(p):
        p = clean.as_clean(p)
        return _lib.CleanPar(*[getattr(p, f) for f in clean.FIELDS])

    def set_batch_clean(self, params=None):
        """Lane cleaning from the next u16 or view begin on (hpe_set_batch_clean): params[b]
        (hpe.clean.Clean or anything as_clean takes) are lane b's; None turns it off.  During a
        cleaned live batch, parameters for the same lanes apply from the next frame cleaned."""
        if params is None:
            self.check(self.lib.hpe_set_batch_clean(self._h, 0, None))
            return
        tab = (_lib.CleanPar * max(len(params), 1))(*[self._clean_par(p) for p in params])
        self.check(self.lib.hpe_set_batch_clean(self._h, len(params), tab))

    def clean_depth_u16(self, frame_u16, params, view_=None):
        """The cleaning rule on one host frame by the batch's kernel (hpe_clean_depth_u16;
        synchronises): frame_u16 is a 240x320 uint16 frame, or with view_ the view's
        (height, pitch) camera frame; returns the cleaned 240x320 uint16 frame, equal to
        hpe.clean.clean on the (reduced) frame."""
        f = np.asarray(frame_u16)
        if f.dtype != np.uint16:
            raise TypeError(f"clean_depth_u16 takes uint16 frames, got {f.dtype}")
        f = np.ascontiguousarray(f)
        v = None if view_ is None else view.as_view(view_)
        need = IMG_H * IMG_W if v is None else v.pitch * v.height
        if f.size != need:
            raise ValueError(f"a frame of {f.size} pixels, {need} expected")
        vs = None if v is None else _lib.View(*[getattr(v, k) for k in view.FIELDS])
        par = self._clean_par(params)
        out = np.empty((IMG_H, IMG_W), dtype=np.uint16)
        self.check(self.lib.hpe_clean_depth_u16(
            self._h, C.c_void_p(f.ctypes.data), None if vs is None else C.byref(vs),
            C.byref(par), C.c_void_p(out.ctypes.data)))
        return out

    def batch_clean_readback(self, parity, lane):
        """Lane `lane`'s cleaned 240x320 uint16 frame of buffer parity `parity`
        (hpe_batch_clean_readback; synchronises)."""
        out = np.empty((IMG_H, IMG_W), dtype=np.uint16)
        self.check(self.lib.hpe_batch_clean_readback(self._h, int(parity), int(lane),
                                                     C.c_void_p(out.ctypes.data)))
        return out

    def batch_wave_wpp(self, num_p, B) -> int:
        """Waves per particle (1 or 2) of a wave-form batch of B lanes of num_p particles: the
        forced HPE_PSO_WPP of the context, else 2 while B * num_p <= 1024 and 1 beyond."""
        rc = self.lib.hpe_batch_wave_wpp(self._h, int(num_p), int(B))
        if rc < 0:
            self.check(rc)
        return rc

    # ---- multi-GPU subswarms: the library's own per-frame exchange (hpe_subswarm_init)
    def subswarm_init(self, uid: bytes, nranks: int, rank: int):
        """Join the RCCL communicator named by uid (hpe.subswarm_unique_id() on rank 0, shared
        with every rank); collective.  Every tracked frame then ends with the all-gather of
        {bestp, cost} over the ranks and the best-of-N pick, inside the frame's graph."""
        b = (C.c_ubyte * _lib.SUBSWARM_ID_BYTES).from_buffer_copy(bytes(uid))
        self.check(self.lib.hpe_subswarm_init(self._h, b, int(nranks), int(rank)))

    def subswarm_init_scripted(self, script, rank: int):
        """The exchange over a scripted transport, which communicates with nobody (one GPU,
        one process, no RCCL): script is a (frames, nranks, 27) float64 array, and exchange k
        puts rows w != rank of script[k] where the all-gather would have put the peers'
        {bestp, cost}.  Loading a script of the live one's shape rewinds the exchange counter
        and keeps the captured graphs."""
        s = np.ascontiguousarray(script, dtype=np.float64)
        if s.ndim != 3 or s.shape[2] != 27:
            raise ValueError("script must be a (frames, nranks, 27) array")
        self.check(self.lib.hpe_subswarm_init_scripted(self._h, int(s.shape[1]), int(rank),
                                                       ptr(s, C.c_double), int(s.shape[0])))

    def subswarm_enable(self, on, direct=False):
        """Suspend (False) / resume (True) the exchange; direct=True resumes it with direct
        launches instead of captured graphs (the library's own fallback form)."""
        self.check(self.lib.hpe_subswarm_enable(self._h, (2 if direct else 1) if on else 0))

    def subswarm_fini(self):
        self.check(self.lib.hpe_subswarm_fini(self._h))

    def subswarm_info(self, gathered=False):
        """{"nranks", "rank", "rccl_version", "in_graphs"[, "gathered": (nranks, 27) rows]}."""
        n = C.c_int32(0); r = C.c_int32(0); v = C.c_int32(0); ig = C.c_int32(0)
        self.check(self.lib.hpe_subswarm_info(self._h, C.byref(n), C.byref(r), C.byref(v),
                                              C.byref(ig), None))
        out = {"nranks": n.value, "rank": r.value, "rccl_version": v.value,
               "in_graphs": bool(ig.value)}
        if gathered and n.value:
            g = np.zeros((n.value, 27))
            self.check(self.lib.hpe_subswarm_info(self._h, None, None, None, None,
                                                  ptr(g, C.c_double)))
            out["gathered"] = g
        return out

    def graph_captures(self) -> int:
        n = C.c_uint64(0)
        self.check(self.lib.hpe_graph_captures(self._h, C.byref(n)))
        return n.value

    def frame_readback(self, slot):
        depth = np.zeros((IMG_H, IMG_W)); dt = np.zeros((IMG_H, IMG_W), dtype=np.float32)
        cloud = np.zeros((IMG_H * IMG_W, 3)); n = C.c_int32(0)
        scale = C.c_double(0); dtmax = C.c_double(0)
        self.check(self.lib.hpe_frame_readback(self._h, slot, ptr(depth, C.c_double),
                                               ptr(dt, C.c_float), ptr(cloud, C.c_double),
                                               C.byref(n), C.byref(scale), C.byref(dtmax)))
        return dict(depth_cm=depth, dt=dt, cloud=cloud[:n.value].copy(), scale=scale.value,
                    dtmax=dtmax.value)

    def pipe_readback(self, parity):
        """frame_readback of the pipeline's prepared-frame buffer `parity` (frame f of a
        pipelined or resident raw sequence is prepared into buffer f & 1)."""
        depth = np.zeros((IMG_H, IMG_W)); dt = np.zeros((IMG_H, IMG_W), dtype=np.float32)
        cloud = np.zeros((IMG_H * IMG_W, 3)); n = C.c_int32(0)
        scale = C.c_double(0); dtmax = C.c_double(0)
        self.check(self.lib.hpe_pipe_readback(self._h, int(parity), ptr(depth, C.c_double),
                                              ptr(dt, C.c_float), ptr(cloud, C.c_double),
                                              C.byref(n), C.byref(scale), C.byref(dtmax)))
        return dict(depth_cm=depth, dt=dt, cloud=cloud[:n.value].copy(), scale=scale.value,
                    dtmax=dtmax.value)

    def render_depth(self, theta, focal=241.42):
        th = _lib.as_f64(theta, (26,))
        out = np.zeros((IMG_H, IMG_W), dtype=np.float32)
        self.check(self.lib.hpe_render_depth(self._h, ptr(th, C.c_double), focal,
                                             ptr(out, C.c_float)))
        return out


def subswarm_unique_id() -> bytes:
    """RCCL's ncclGetUniqueId (128 bytes) for hpe_subswarm_init; call on one rank."""
    lib = _lib.load()
    b = (C.c_ubyte * _lib.SUBSWARM_ID_BYTES)()
    rc = lib.hpe_subswarm_unique_id(b)
    if rc != 0:
        raise HpeError(f"hpe_subswarm_unique_id failed ({rc}): RCCL not loadable?")
    return bytes(b)


def preprocess_depth(depth_mm, to_cm=True, downsample=True, focal=241.42):
    """observedmodel preprocessing (host C++ in libhpe.so; no GPU needed)."""
    lib = _lib.load()
    d = np.ascontiguousarray(depth_mm, dtype=np.float32).reshape(IMG_H, IMG_W)
    depth_cm = np.zeros((IMG_H, IMG_W)); dt = np.zeros((IMG_H, IMG_W), dtype=np.float32)
    cloud = np.zeros((IMG_H * IMG_W, 3)); n = C.c_int32(0)
    scale = C.c_double(0); dtmax = C.c_double(0); K = np.zeros(9)
    rc = lib.hpe_preprocess_depth(ptr(d, C.c_float), int(to_cm), int(downsample), focal,
                                  ptr(depth_cm, C.c_double), ptr(dt, C.c_float),
                                  ptr(cloud, C.c_double), C.byref(n), C.byref(scale),
                                  C.byref(dtmax), ptr(K, C.c_double))
    if rc != 0:
        raise HpeError(f"hpe_preprocess_depth failed ({rc})")
    return dict(depth_cm=depth_cm, dt=dt, cloud=cloud[:n.value].copy(), scale=scale.value,
                dtmax=dtmax.value, K=K.reshape(3, 3))


class handmodel:
    """handmodel(h_geo, h_spacing, tb_spheres, fg_spheres, h_CMC, sphR)
    (handmodel.h:9-10): lengths/radii in cm."""

    def __init__(self, h_geo, h_spacing, tb_spheres, fg_spheres, h_CMC, sphR, device=0):
        p = _lib.HandParams()
        p.geo_cm[:] = [float(x) for x in np.asarray(h_geo).ravel()]
        p.radii_cm[:] = [float(x) for x in np.asarray(sphR).ravel()]
        p.cmc_deg[:] = [float(x) for x in np.asarray(h_CMC).ravel()]
        p.spacing_cm[:] = [float(x) for x in np.asarray(h_spacing).ravel()]
        p.tb_spheres[:] = [int(x) for x in np.asarray(tb_spheres).ravel()]
        p.fg_spheres[:] = [int(x) for x in np.asarray(fg_spheres).ravel()]
        self.params = p
        self.ctx = Context(p, device)
        self.spheres_radii = np.asarray(sphR, dtype=np.float64).copy()
        self.hand_joints = np.zeros((21, 3))

    def get_radii(self):
        return self.spheres_radii

    def build_hand_model(self, h_theta, sphere_centres=None):
        """handmodel.cpp:259-298; fills sphere_centres (48,3) in place if given."""
        th = _lib.as_f64(h_theta, (1, 26))
        S = np.zeros((1, 48, 3)); J = np.zeros((1, 21, 3))
        self.ctx.check(self.ctx.lib.hpe_build_spheres(self.ctx.h, ptr(th, C.c_double), 1,
                                                      ptr(S, C.c_double), ptr(J, C.c_double)))
        self.hand_joints = J[0]
        if sphere_centres is not None:
            sphere_centres[...] = S[0]
        return S[0]

    def build_batch(self, thetas):
        th = _lib.as_f64(thetas).reshape(-1, 26)
        S = np.zeros((len(th), 48, 3)); J = np.zeros((len(th), 21, 3))
        self.ctx.check(self.ctx.lib.hpe_build_spheres(self.ctx.h, ptr(th, C.c_double), len(th),
                                                      ptr(S, C.c_double), ptr(J, C.c_double)))
        return S, J


def reference_geometry():
    """(geo_cm (20,), radii_cm (48,)) of the reference hand, from the committed misc/*.dat
    values."""
    d = json.loads((Path(__file__).parent / "hand_subject1.json").read_text())
    return np.array(d["hgeo_mm"]) / 10.0, np.array(d["rad_mm"]) / 10.0


def reference_hand(device=0):
    """The hand of test_full (testmodel.cpp:33-52) from the committed misc/*.dat values."""
    geo, rad = reference_geometry()
    return handmodel(geo, SPACING, TB_SPHERES, FG_SPHERES, CMC, rad, device=device)


def scaled_hand_params(scale, radius_scale=None) -> _lib.HandParams:
    """The reference hand's parameters with geo_cm times scale and radii_cm times radius_scale
    (default: scale); CMC, spacing and the sphere counts are the reference's.  No context."""
    geo, rad = reference_geometry()
    rs = scale if radius_scale is None else radius_scale
    p = _lib.HandParams()
    p.geo_cm[:] = [float(x) for x in geo * float(scale)]
    p.radii_cm[:] = [float(x) for x in rad * float(rs)]
    p.cmc_deg[:] = CMC
    p.spacing_cm[:] = SPACING
    p.tb_spheres[:] = TB_SPHERES
    p.fg_spheres[:] = FG_SPHERES
    return p


def scaled_hand(scale, radius_scale=None, device=0):
    """The reference hand with its segment lengths scaled by `scale` and its sphere radii by
    radius_scale (default: scale) -- another subject's hand size for Context.set_batch_hands.
    Only geometry and radii change, so oracle_np.Hand(geo, rad) / oracle.hand(geo, rad) mirror
    it."""
    p = scaled_hand_params(scale, radius_scale)
    return handmodel(np.array(p.geo_cm[:]), SPACING, TB_SPHERES, FG_SPHERES, CMC,
                     np.array(p.radii_cm[:]), device=device)


class observedmodel:
    """observedmodel (observedmodel.h): .bin depth frames -> cloud, depth, DT, scale."""

    _token = 0

    def __init__(self):
        self.path = "../handModelling/Release_2014_5_28/Subject1/"
        self.filename = "000001_depth.bin"
        self.imgW, self.imgH = 240, 320
        self.to_cm, self.downsample, self.focal_len = True, False, 241.42
        self._obs = None

    def init_observation(self, dpath, dfname, mm_to_cm, imW, imH, foclen, downsampling):
        self.path, self.filename = dpath, dfname
        self.imgW, self.imgH = imW, imH
        self.to_cm, self.focal_len, self.downsample = mm_to_cm, foclen, downsampling
        self.load_data()

    def load_data(self):
        """observedmodel.cpp:272-310: headerless float32 mm, 240 x 320 row-major."""
        p = Path(self.path) / self.filename
        if not p.exists():
            raise FileNotFoundError(f"error: open file for input failed! ({p})")
        self.set_depth_mm(np.fromfile(p, dtype=np.float32))

    def set_depth_mm(self, depth_mm):
        """Use an in-memory frame (e.g. a synthetic one) instead of a .bin file."""
        self._obs = preprocess_depth(depth_mm, self.to_cm, self.downsample, self.focal_len)
        observedmodel._token += 1
        self.token = observedmodel._token

    def next_frame(self, name):
        self.filename = name
        self.load_data()
        return self

    def get_ptncloud(self): return self._obs["cloud"]
    def get_depthmap(self): return self._obs["depth_cm"]
    def get_disttran(self): return self._obs["dt"]
    def get_camera_mat(self): return self._obs["K"]
    def get_img_scale(self): return self._obs["scale"]
    def get_dtmax(self): return self._obs["dtmax"]


class costfunc:
    """costfunc(handmodel*, observedmodel*) (costfunc.h:25-41)."""

    def __init__(self, handM: handmodel, observed: observedmodel):
        self.hand, self.observation = handM, observed
        self.ctx = handM.ctx

    def _sync_frame(self):
        o = self.observation
        if self.ctx.frame_token != o.token:
            d = o._obs
            self.ctx.store_frame(0, d["depth_cm"], d["dt"], d["cloud"], d["scale"],
                                 d["dtmax"], d["K"])
            self.ctx.select_frame(0)
            self.ctx.frame_token = o.token

    def cal_cost(self, theta):
        return float(self.cal_cost_batch(np.asarray(theta).reshape(1, 26))[0])

    def cal_cost_batch(self, thetas, with_collision=False, return_match=False):
        """The OpenMP particle loops of PSO.cpp:748,848 as one launch."""
        self._sync_frame()
        th = _lib.as_f64(thetas).reshape(-1, 26)
        cost = np.zeros(len(th))
        n = len(self.observation.get_ptncloud())
        m = np.zeros((len(th), n), dtype=np.int32) if return_match else None
        self.ctx.check(self.ctx.lib.hpe_eval_costs(
            self.ctx.h, ptr(th, C.c_double), len(th), int(with_collision),
            ptr(cost, C.c_double), ptr(m, C.c_int32) if m is not None else None))
        return (cost, m) if return_match else cost

    def cal_cost2(self, theta, matchId, compute_corr, debug=False):
        """costfunc.cpp:31-86; matchId (int32, len N) is filled in place when
        compute_corr, read otherwise."""
        self._sync_frame()
        th = _lib.as_f64(theta, (26,))
        if matchId.dtype != np.int32 or not matchId.flags.c_contiguous:
            raise TypeError("matchId must be a contiguous int32 array")
        cost = C.c_double(0); terms = np.zeros(3)
        self.ctx.check(self.ctx.lib.hpe_cal_cost2(self.ctx.h, ptr(th, C.c_double),
                                                  ptr(matchId, C.c_int32), int(compute_corr),
                                                  C.byref(cost), ptr(terms, C.c_double)))
        if debug:
            print(terms[0]); print(terms[1]); print(terms[2], "\n")
        self.last_terms = terms
        return cost.value

    def gnd_truth_err(self, gnd_truth, frame):
        """costfunc.cpp:476-507: wrist + finger-tip error (mm) of the hand_joints left by the
        last build_hand_model against row `frame` of gnd_truth (frames x 63)."""
        return gnd_truth_err(self.hand.hand_joints, np.asarray(gnd_truth)[frame])

    # ---- term-level API on a sphere matrix (costfunc.cpp:130-377), one launch each
    def _sphere_terms(self, spheres, matchId=None):
        self._sync_frame()
        S = _lib.as_f64(spheres, (48, 3))
        n = len(self.observation.get_ptncloud())
        corr = matchId is None
        m = np.zeros(n, dtype=np.int32) if corr else np.ascontiguousarray(matchId, dtype=np.int32)
        terms = np.zeros(3)
        self.ctx.check(self.ctx.lib.hpe_eval_spheres(self.ctx.h, ptr(S, C.c_double), 1, int(corr),
                                                     ptr(m, C.c_int32), ptr(terms, C.c_double)))
        return terms, m

    def _same_cloud(self, ptncloud):
        own = self.observation.get_ptncloud()
        if ptncloud is not own and not np.array_equal(np.asarray(ptncloud), own):
            raise ValueError("the device path evaluates the observation's own point cloud")

    def compute_correspondences(self, ptns, sphM, matchId):
        """costfunc.cpp:306-343: nearest sphere centre per cloud point (BFMatcher, fp32,
        first index on ties).  matchId (int32, len N) is filled in place."""
        self._same_cloud(ptns)
        _, m = self._sphere_terms(sphM)
        matchId[...] = m
        return matchId

    def align_models(self, spheresR, spheresM, ptncloud, matchId):
        """costfunc.cpp:346-377: (48/N) sum (|p - S[m]| - r[m])^2 with the given matchId."""
        self._same_cloud(ptncloud)
        if not np.array_equal(np.asarray(spheresR, dtype=np.float64), self.hand.spheres_radii):
            raise ValueError("the device path uses the hand's own radii")
        return float(self._sphere_terms(spheresM, matchId)[0][0])

    def depth_penalty(self, cam_mat, depthmp, spheres, disttrans, scale):
        """costfunc.cpp:227-304 on the observation's depth / DT / scale.  Like the
        reference it un-negates y and z of `spheres` in place (:249)."""
        val = float(self._sphere_terms(spheres)[0][1])
        spheres[:, 1:3] *= -1
        return val

    def self_collision_penalty(self, spheresM, spheresR):
        """costfunc.cpp:130-197: adjacent-digit sphere overlap penalty."""
        return float(self._sphere_terms(spheresM)[0][2])


def gnd_truth_err(hand_joints, gt_row):
    """costfunc.cpp:476-507 for one frame: gt_row holds 63 values (joint j at 3j..3j+2, mm);
    hand_joints is the (21, 3) cm matrix of build_hand_model (handmodel.cpp:291-296)."""
    gt = np.asarray(gt_row, dtype=np.float64).reshape(21, 3)
    hj = np.asarray(hand_joints, dtype=np.float64) * 10.0
    hj[:, 1:3] *= -1
    e = gt - hj
    d = [float(np.sqrt((e[j, 0] * e[j, 0] + e[j, 1] * e[j, 1]) + e[j, 2] * e[j, 2]))
         for j in (0, 4, 8, 12, 16, 20)]
    return ((d[0] + d[2]) + d[4]) + ((d[1] + d[3]) + d[5])


class PSO:
    """PSO (PSO.h:15-72)."""

    def __init__(self):
        self.w, self.c1, self.c2 = 0.7298, 1.49618, 1.49618  # PSO.cpp:29-34
        self.maxiter, self.minstep, self.minfunc = 100, 1e-6, 1e-6
        self.theta_max = self.theta_min = self.theta_std = None
        self.seed = 1000  # arma_rng::set_seed(1000), PSO.cpp:722

    def set_pso_params(self, upperbound, lowerbound, std, omega, phip, phig, maxIter,
                       minStep, minFunc):
        self.theta_max = _lib.as_f64(upperbound, (26,)).copy()
        self.theta_min = _lib.as_f64(lowerbound, (26,)).copy()
        self.theta_std = _lib.as_f64(std, (26,)).copy()
        self.w, self.c1, self.c2 = omega, phip, phig
        self.maxiter, self.minstep, self.minfunc = maxIter, minStep, minFunc

    def dim_restore(self, theta_in, theta_out):
        """PSO.cpp:160-180: 22 -> 26 DOF in place, each finger's DIP = 2/3 of its PIP
        (rows 13, 17, 21, 25); theta_out must hold 26 values."""
        ti = np.asarray(theta_in, dtype=np.float64).ravel()
        if ti.size < 22 or np.asarray(theta_out).size < 26:
            raise IndexError("Mat::rows(): indices out of bounds or incorrectly used")
        theta_out[0:13] = ti[0:13]
        theta_out[13] = 2. / 3 * ti[12]
        for f in range(3):  # middle, ring, little
            o, i = 14 + 4 * f, 13 + 3 * f
            theta_out[o:o + 3] = ti[i:i + 3]
            theta_out[o + 3] = 2. / 3 * ti[i + 2]

    def _push(self, ctx):
        ctx.check(ctx.lib.hpe_set_pso_params(
            ctx.h, ptr(self.theta_max, C.c_double), ptr(self.theta_min, C.c_double),
            ptr(self.theta_std, C.c_double), self.w, self.c1, self.c2, int(self.maxiter),
            self.minstep, self.minfunc))
        ctx.check(ctx.lib.hpe_set_seed(ctx.h, C.c_uint64(self.seed)))

    def pso_evolve(self, optfunc: costfunc, x0, num_particles, bestp):
        """PSO.cpp:717-886: bestp (26,) filled in place; returns 1."""
        ctx = optfunc.ctx
        optfunc._sync_frame()
        self._push(ctx)
        x = _lib.as_f64(x0, (26,))
        out = np.zeros(26); bc = C.c_double(0)
        ctx.check(ctx.lib.hpe_pso_evolve(ctx.h, ptr(x, C.c_double), int(num_particles),
                                         ptr(out, C.c_double), C.byref(bc)))
        bestp[...] = out
        self.last_gbest_cost = bc.value
        return 1

    def pso_optimise(self, optfunc: costfunc, x0, num_p, bestp):
        """PSO.cpp:539-712 (descent + global-best PSO with omega / phip / phig of
        set_pso_params): bestp (26,) filled in place; returns 1.  The gbest cost after each
        generation is kept in last_optimise_trace."""
        ctx = optfunc.ctx
        optfunc._sync_frame()
        self._push(ctx)
        x = _lib.as_f64(x0, (26,))
        out = np.zeros(26); bc = C.c_double(0)
        G = max(self.maxiter - 1, 0)
        tr = np.zeros(max(G, 1))
        ctx.check(ctx.lib.hpe_pso_optimise(ctx.h, ptr(x, C.c_double), int(num_p),
                                           ptr(out, C.c_double), C.byref(bc),
                                           ptr(tr, C.c_double), G))
        bestp[...] = out
        self.last_gbest_cost = bc.value
        self.last_optimise_trace = tr[:G]
        return 1

    def trace(self, optfunc: costfunc):
        G = self.maxiter - 1
        g = np.zeros(max(G, 1)); cnt = np.zeros(max(G, 1), dtype=np.int32)
        topo = np.zeros(max(G, 1), dtype=np.int32)
        ctx = optfunc.ctx
        ctx.check(ctx.lib.hpe_pso_trace(ctx.h, ptr(g, C.c_double), ptr(cnt, C.c_int32),
                                        ptr(topo, C.c_int32), G))
        return g[:G], cnt[:G], topo[:G]

    def refine_init_pose(self, x0, optfunc: costfunc):
        """PSO.cpp:216-266: x0 (26,) refined in place."""
        ctx = optfunc.ctx
        optfunc._sync_frame()
        x = _lib.as_f64(x0, (26,)).copy()
        ev = C.c_int32(0)
        ctx.check(ctx.lib.hpe_refine_init_pose(ctx.h, ptr(x, C.c_double), C.byref(ev)))
        x0[...] = x
        self.last_refine_evals = ev.value

    def track_frame(self, optfunc: costfunc, x0, num_particles, refine=True):
        """testmodel.cpp:126-138 in one call: refine, pso_evolve, cal_cost(bestp);
        x0 <- bestp in place; returns the frame cost."""
        ctx = optfunc.ctx
        optfunc._sync_frame()
        self._push(ctx)
        x = _lib.as_f64(x0, (26,)).copy()
        c = C.c_double(0)
        ctx.check(ctx.lib.hpe_track_frame(ctx.h, int(num_particles), int(refine),
                                          ptr(x, C.c_double), C.byref(c)))
        x0[...] = x
        return c.value
