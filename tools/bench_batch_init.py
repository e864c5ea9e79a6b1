"""Time the initialisation of B lanes at test_full's settings (P = 32, maxiter = 200,
250-point frames), three ways in one session with alternating legs:

  (a) parent   another build of libhpe.so (--parent-lib: the parent commit's, built into a side
               directory and loaded by path) making B consecutive hpe_pso_optimise calls -- the
               only way before hpe_pso_optimise_batch;
  (b) batch    this build's hpe_pso_optimise_batch, bracketed by events on the context's stream
               (device time) and by the host clock around the call and a synchronisation;
  (c) single   this build's B consecutive hpe_pso_optimise calls: its kernels are the parent's,
               so it must sit inside (a)'s run-to-run spread.

Each leg runs once discarded, then --runs times; the median and the extremes are reported, one
JSON line per B, appended to --out.  To build the parent's library:

  git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/hand-pose-estimation_amd libhpe.so

Without --parent-lib, leg (a) is left out and the line says so.
"""
import argparse
import ctypes as C
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
from hpe import _lib, synth  # noqa: E402

USED = ("hpe_create", "hpe_destroy", "hpe_last_error", "hpe_store_frame", "hpe_select_frame",
        "hpe_set_pso_params", "hpe_set_seed", "hpe_pso_optimise", "hpe_sync", "hpe_stream",
        "hpe_render_depth")


def open_lib(path):
    """A build of libhpe.so by path, with the signatures of the entry points used here (a build
    from before the lane calls lacks them: they are optional)."""
    lib = C.CDLL(str(path))
    for name in USED + ("hpe_pso_optimise_batch",):
        if name in USED or hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = _lib.SIGNATURES[name]
    return lib


class Ctx:
    """One context of one build, on the reference hand, with the frames stored in slots 0.."""

    def __init__(self, lib, maxiter):
        self.lib, self.h = lib, C.c_void_p()
        p = hpe.scaled_hand_params(1.0)
        self.ok(lib.hpe_create(C.byref(self.h), 0, C.byref(p)))
        ub, lb, sd = (_lib.as_f64(a, (26,)) for a in hpe.reference_bounds())
        d = lambda a: _lib.ptr(a, C.c_double)
        self.ok(lib.hpe_set_pso_params(self.h, d(ub), d(lb), d(sd), 0.7298, 1.49618, 1.49618,
                                       maxiter, 1e-8, 1e-8))
        self.ok(lib.hpe_set_seed(self.h, C.c_uint64(1000)))
        self.G = maxiter - 1

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError("%d: %s" % (rc, self.lib.hpe_last_error(self.h).decode()))

    def render(self, theta):
        out = np.zeros((240, 320), dtype=np.float32)
        th = _lib.as_f64(theta, (26,))
        self.ok(self.lib.hpe_render_depth(self.h, _lib.ptr(th, C.c_double), 241.42,
                                          _lib.ptr(out, C.c_float)))
        return out

    def store(self, slot, o):
        cloud = np.ascontiguousarray(o["cloud"], dtype=np.float64)
        f = _lib.Frame(_lib.ptr(o["depth_cm"], C.c_double), _lib.ptr(o["dt"], C.c_float),
                       _lib.ptr(cloud, C.c_double), len(cloud), float(o["scale"]), float(o["dtmax"]),
                       (C.c_double * 9)(*np.asarray(o["K"], dtype=np.float64).ravel()))
        self.ok(self.lib.hpe_store_frame(self.h, slot, C.byref(f)))

    def singles(self, P, x0s):
        """B consecutive select_frame + hpe_pso_optimise: (host ms, the {bestp, cost} rows)."""
        out = np.zeros((len(x0s), 27))
        bc = C.c_double(0)
        t0 = time.perf_counter()
        for b, x in enumerate(x0s):
            self.ok(self.lib.hpe_select_frame(self.h, b))
            self.ok(self.lib.hpe_pso_optimise(self.h, _lib.ptr(x, C.c_double), P,
                                              _lib.ptr(out[b], C.c_double), C.byref(bc), None, 0))
            out[b, 26] = bc.value
        return (time.perf_counter() - t0) * 1e3, out

    def batch(self, P, x0s):
        """hpe_pso_optimise_batch: (device ms between stream events, host ms, the rows)."""
        B = len(x0s)
        rows = np.zeros((B, 27))
        rows[:, :26] = x0s
        st = torch.from_numpy(rows).to("cuda:0")
        slots = (C.c_int32 * B)(*range(B))
        stream = torch.cuda.ExternalStream(self.lib.hpe_stream(self.h))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        self.ok(self.lib.hpe_pso_optimise_batch(self.h, P, B, C.c_void_p(st.data_ptr()), slots, None))
        e1.record(stream)
        self.ok(self.lib.hpe_sync(self.h))
        host = (time.perf_counter() - t0) * 1e3
        e1.synchronize()
        return e0.elapsed_time(e1), host, st.cpu().numpy()

    def close(self):
        self.lib.hpe_destroy(self.h)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libhpe.so")
    ap.add_argument("--lanes", default="1,2,4,8,16")
    ap.add_argument("--num-p", type=int, default=32)
    ap.add_argument("--maxiter", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_init" / "bench_batch_init.jsonl"))
    a = ap.parse_args()
    lanes = [int(x) for x in a.lanes.split(",")]
    if a.runs < 1 or any(not 1 <= b <= _lib.BATCH_MAX for b in lanes):
        ap.error("--runs >= 1 and lanes in 1..%d" % _lib.BATCH_MAX)
    this = Ctx(open_lib(_lib.LIB_PATH), a.maxiter)
    parent = Ctx(open_lib(a.parent_lib), a.maxiter) if a.parent_lib else None
    Bmax = max(lanes)
    poses = synth.trajectory(Bmax + 1, seed=0)
    x0s = [np.ascontiguousarray(poses[b], dtype=np.float64) for b in range(Bmax)]
    for b in range(Bmax):  # lane b: the frame after its start pose, 250 points
        o = hpe.preprocess_depth(this.render(poses[b + 1]), True, True, 241.42)
        for c in (this, parent):
            if c:
                c.store(b, o)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for B in lanes:
        xs = x0s[:B]
        legs = {"batch_dev": [], "batch_host": [], "single": [], "parent": []}
        rows = {}
        for r in range(a.runs + 1):  # run 0 is the discarded warm-up of every leg
            if parent:
                ms, rows["parent"] = parent.singles(a.num_p, xs)
                if r:
                    legs["parent"].append(ms)
            dev, host, rows["batch"] = this.batch(a.num_p, xs)
            ms, rows["single"] = this.singles(a.num_p, xs)
            if r:
                legs["batch_dev"].append(dev)
                legs["batch_host"].append(host)
                legs["single"].append(ms)
        line = {"bench": "batch_init", "B": B, "num_p": a.num_p, "maxiter": a.maxiter,
                "cloud_points": 250,
                "batch_equals_single": bool(np.array_equal(rows["batch"], rows["single"])),
                "batch_dev": stats(legs["batch_dev"]), "batch_host": stats(legs["batch_host"]),
                "single": stats(legs["single"])}
        if parent:
            line["parent"] = stats(legs["parent"])
            line["single_equals_parent"] = bool(np.array_equal(rows["single"], rows["parent"]))
            line["speedup_vs_parent"] = line["parent"]["median_ms"] / line["batch_host"]["median_ms"]
        else:
            line["parent"] = None  # no --parent-lib: leg (a) was not run
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    this.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
