"""What tests/test_gpu_batch_seeds.py and tests/test_gpu_batch_groups.py share: the frames, the
single-sequence yardsticks and the batch under test.  Not a test module.

Sizes: P = 24 and P = 40 (either side of the 32 gmin shards, a multiple of neither), maxiter 6
(G = 5), 250-point clouds, 3 frames per stream.  Frames come from hand_data.trajectory and
oracle_np.render_depth_mm; lane b's seed is 1000 + b.

The yardstick uses no code of lane seeds or groups.  There is one context per distinct (seed,
form, waves per particle, hand), seeded with hpe_set_seed; frame f of a lane is the
single-sequence call the batch call mirrors on that one frame, run from the lane's row x_{f-1}
(f = 0: the row the caller gave it), and x_f is hpe.dist.pick_best over the group's own rows.
Steps are computed once per (context, call, frame, start row) and shared.
"""
import os

import numpy as np

P_SIZES = (24, 40)
MAXITER, NF, FOCAL = 6, 3, 241.42
SENTINEL = -7.0


def seeds_for(B):
    return [1000 + b for b in range(B)]


def same(a, b):
    """Bit equality, NaNs included (as tests/test_gpu_subswarm_world.py's _same)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make_hand(name):
    import hpe
    if name == "A":
        return hpe.reference_hand(device=0)
    assert name == "S"
    return hpe.scaled_hand(0.9, 0.85)


def _create(name, form, wpp):
    saved = {k: os.environ.pop(k, None) for k in ("HPE_PSO_FORM", "HPE_PSO_WPP")}
    try:
        if form:
            os.environ["HPE_PSO_FORM"] = form
        if wpp:
            os.environ["HPE_PSO_WPP"] = str(wpp)
        return make_hand(name)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Ctx:
    """One context: hand `name`, created under HPE_PSO_FORM / HPE_PSO_WPP if given, PSO seed
    `seed` (hpe_set_seed)."""

    def __init__(self, pool, name="A", form=None, wpp=None, seed=1000):
        import hpe
        import torch
        self.hpe, self.torch, self.pool = hpe, torch, pool
        self.hand = _create(name, form, wpp)
        self.ctx = self.hand.ctx
        self.lib = self.ctx.lib
        ub, lb, sd = hpe.reference_bounds()
        self.pso = hpe.PSO()
        self.pso.seed = seed
        self.pso.set_pso_params(ub, lb, sd, 0.7298, 1.49618, 1.49618, MAXITER, 1e-8, 1e-8)
        self.pso._push(self.ctx)
        self.x0 = np.asarray(hpe.X0, dtype=np.float64)
        self.st1 = torch.zeros(27, dtype=torch.float64, device="cuda:0")
        self.bufs = {}
        self.slots = {}
        self.next_slot = 8
        self.sync()

    def sync(self):
        self.ctx.check(self.lib.hpe_sync(self.ctx.h))

    def end_live(self):
        """End a live batch in progress, if any, by one last track call into rows for the largest
        batch (a finished test leaves none: then nothing runs)."""
        try:
            self.ctx.batch_pending()
        except self.hpe.HpeError:
            return
        st, _ = self.bufs_for(self.hpe._lib.BATCH_MAX, 1, "end")
        self.ctx.track_batch_pipelined(P_SIZES[0], 1, st.data_ptr(), None)
        self.sync()

    def slot0(self, stream):
        if stream not in self.slots:
            self.slots[stream] = self.next_slot
            for f, d in enumerate(self.pool.frames(stream)):
                self.ctx.prepare_frame(self.next_slot + f, d)
            self.next_slot += NF
            self.sync()
        return self.slots[stream]

    # ---- the yardstick: one frame by the single-sequence call, from row x
    def step(self, kind, P, stream, f, x, refine=1, window=None):
        self.st1.copy_(self.torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)))
        self.torch.cuda.synchronize()
        d = self.pool.frames(stream)[f]
        if window is not None:
            from hpe import window as W
            d = W.apply(d, window)
        if kind == "prepared":
            assert window is None
            self.ctx.track_sequence(P, refine, self.st1.data_ptr(), self.slot0(stream) + f, 1, 1)
        elif kind == "raw":
            raw = self.torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0")
            self.ctx.track_raw_sequence(P, refine, self.st1.data_ptr(), raw.data_ptr(), 1,
                                        frames_per_graph=1)
        else:
            self.ctx.pipeline_begin(d)
            self.ctx.track_pipelined(P, refine, self.st1.data_ptr(), None)
        self.sync()
        return self.st1.cpu().numpy().copy()

    # ---- the batch under test
    def bufs_for(self, B, n, tag=None):
        t = self.torch
        if (B, n, tag) not in self.bufs:
            self.bufs[(B, n, tag)] = (t.zeros((B, 27), dtype=t.float64, device="cuda:0"),
                                      t.empty((B, n, 27), dtype=t.float64, device="cuda:0"))
        return self.bufs[(B, n, tag)]

    def batch(self, kind, P, streams, starts, n=NF, form="auto", K=2, tag=None, refine=1,
              after=None):
        """The batch call over the lanes' streams from the rows `starts` (B x 27).  prepared / raw:
        one call of n frames -> (hist B x n x 27, states B x 27); live: a begin and n track
        calls -> the states after every frame, n x B x 27.  after(f): called after frame f of a
        live batch has been synchronised (own rows, reports)."""
        B = len(streams)
        st, hist = self.bufs_for(B, n, tag)
        st.copy_(self.torch.from_numpy(np.ascontiguousarray(starts, dtype=np.float64)))
        hist.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        self.ctx.set_batch_form(form)
        try:
            if kind == "prepared":
                self.ctx.track_batch(P, refine, st.data_ptr(), [self.slot0(s) for s in streams], n, K,
                                     hist.data_ptr())
            elif kind == "raw":
                self.ctx.track_raw_batch(P, refine, st.data_ptr(),
                                         [self.pool.raw(s).data_ptr() for s in streams], n,
                                         frames_per_graph=K, d_hist_ptr=hist.data_ptr())
            else:
                out = []
                fr = [self.pool.frames(s) for s in streams]
                self.ctx.batch_pipeline_begin([x[0] for x in fr])
                for f in range(n):
                    self.ctx.track_batch_pipelined(P, refine, st.data_ptr(),
                                                   [x[f + 1] for x in fr] if f + 1 < n else None)
                    self.sync()
                    out.append(st.cpu().numpy().copy())
                    if after:
                        after(f)
                return np.array(out)
            self.sync()
        finally:
            self.ctx.set_batch_form("auto")
        return hist.cpu().numpy().copy(), st.cpu().numpy().copy()


class Pool:
    def __init__(self):
        self._frames, self._raws, self.ctxs, self.steps = {}, {}, {}, {}
        self.batch_ctxs = {}

    def frames(self, stream):
        """NF frames of hand_data.trajectory(NF, seed=stream) rendered by the numpy oracle."""
        if stream not in self._frames:
            import hand_data
            import oracle_np
            geo, rad = hand_data.geometry_cm()
            hand = oracle_np.Hand(geo, rad)
            self._frames[stream] = [
                np.ascontiguousarray(oracle_np.render_depth_mm(hand, th), dtype=np.float32)
                for th in hand_data.trajectory(NF, seed=stream)]
        return self._frames[stream]

    def raw(self, stream):
        if stream not in self._raws:
            import torch
            self._raws[stream] = torch.from_numpy(np.stack(self.frames(stream))).to("cuda:0")
        return self._raws[stream]

    def start(self, B=1, x0=None):
        import hpe
        x = np.zeros((B, 27))
        x[:, :26] = np.asarray(hpe.X0 if x0 is None else x0, dtype=np.float64)
        return x

    def single(self, seed, form=None, wpp=None, name="A"):
        key = (seed, form, wpp, name)
        if key not in self.ctxs:
            self.ctxs[key] = Ctx(self, name, form, wpp, seed)
        return self.ctxs[key]

    def under_test(self, wpp=None):
        """The context the batches run on: the reference hand, the default seed; wpp forces the
        waves per particle of its wave-form batches (HPE_PSO_WPP, read at hpe_create)."""
        if wpp not in self.batch_ctxs:
            self.batch_ctxs[wpp] = Ctx(self, "A", None, wpp, 1000)
        return self.batch_ctxs[wpp]

    def step(self, kind, P, seed, stream, f, x, form=None, wpp=None, name="A", window=None):
        key = (kind, P, seed, stream, f, np.ascontiguousarray(x).tobytes(), form, wpp, name, window)
        if key not in self.steps:
            self.steps[key] = self.single(seed, form, wpp, name).step(kind, P, stream, f, x,
                                                                       window=window)
        return self.steps[key]

    def yard(self, kind, P, seeds, streams, starts, sizes=None, n=NF, form=None, wpp=None,
             names=None):
        """(own, picked), each n x B x 27: every lane's own result of frame f and the rows after
        the groups' pick (sizes None: every lane a group of its own, the pick the identity)."""
        import torch
        from hpe import dist
        B = len(seeds)
        sizes = [1] * B if sizes is None else sizes
        x = np.array(starts, dtype=np.float64, copy=True)
        own, picked = [], []
        for f in range(n):
            rows = np.stack([self.step(kind, P, seeds[b], streams[b], f, x[b], form, wpp,
                                       names[b] if names else "A") for b in range(B)])
            x, at = rows.copy(), 0
            for z in sizes:
                x[at:at + z] = dist.pick_best(torch.from_numpy(rows[at:at + z])).numpy()
                at += z
            own.append(rows)
            picked.append(x.copy())
        return np.array(own), np.array(picked)

    def close(self):
        for c in list(self.ctxs.values()) + list(self.batch_ctxs.values()):
            c.ctx.close()
