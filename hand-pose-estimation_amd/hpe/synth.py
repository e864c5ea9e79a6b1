"""Synthetic input for bench and smoke runs (no MSRA data exists on the GPU box).

A seeded, smooth 26-DOF pose trajectory starting at test_full's x0
(testmodel.cpp:38-40), rendered by the GPU into 240x320 float32 mm depth frames in the
reference .bin layout (observedmodel.cpp:280-308), preprocessed like next_frame
(observedmodel.cpp:420-430) and stored resident in HBM frame slots.
"""
from __future__ import annotations

import numpy as np

from . import X0, Context, preprocess_depth, reference_bounds


def trajectory(n_frames: int, seed: int = 0, step: float = 0.15,
               revert: float = 0.0) -> np.ndarray:
    """revert > 0 pulls the pose back towards x0 (long sequences stay in view)."""
    rng = np.random.default_rng(seed)
    ub, lb, sd = reference_bounds()
    poses = [X0.copy()]
    vel = np.zeros(26)
    for _ in range(n_frames - 1):
        vel = 0.8 * vel + 0.2 * rng.standard_normal(26) * sd * step
        vel += revert * (X0 - poses[-1])
        poses.append(np.clip(poses[-1] + vel, lb, ub))
    return np.array(poses)


def load_sequence(ctx: Context, n_frames: int, seed: int = 0, downsample: bool = True,
                  focal: float = 241.42, first_slot: int = 0):
    """Render + preprocess + store n_frames into slots first_slot..; returns
    (poses, cloud sizes)."""
    poses = trajectory(n_frames, seed)
    sizes = []
    for f, th in enumerate(poses):
        d = ctx.render_depth(th, focal)
        o = preprocess_depth(d, True, downsample, focal)
        ctx.store_frame(first_slot + f, o["depth_cm"], o["dt"], o["cloud"], o["scale"],
                        o["dtmax"], o["K"])
        sizes.append(len(o["cloud"]))
    return poses, sizes


def _grow(mask: np.ndarray, k: int) -> np.ndarray:
    """The mask dilated k times by the 3x3 square."""
    m = mask.copy()
    for _ in range(k):
        p = np.zeros((m.shape[0] + 2, m.shape[1] + 2), dtype=bool)
        p[1:-1, 1:-1] = m
        m = np.zeros_like(m)
        for dr in range(3):
            for dc in range(3):
                m |= p[dr:dr + mask.shape[0], dc:dc + mask.shape[1]]
    return m


def camera_noise(frame_u16, seed, background: int = 800, flying: float = 0.3,
                 speckle: int = 40, ring: int = 10, jitter: int = 30) -> np.ndarray:
    """What a time-of-flight or structured-light camera makes of a rendered uint16 frame (0: no
    depth), seeded and deterministic; a new array.
    Flying pixels: the share `flying` of the silhouette pixels -- hand pixels with a hole among
    their eight neighbours -- takes a depth between its own and `background` (raw units, behind
    the hand), 20 % to 80 % of the way.
    Speckle: `speckle` single pixels scattered over the holes that lie 2 .. `ring` pixels from the
    hand, at the hand's median depth +- `jitter`: inside any window that holds the hand."""
    f = np.asarray(frame_u16)
    if f.dtype != np.uint16 or f.ndim != 2:
        raise TypeError(f"camera_noise takes 2-D uint16 frames, got {f.dtype}")
    rng = np.random.default_rng(seed)
    out = f.copy()
    on = f > 0
    if not on.any():
        return out
    edge = np.flatnonzero(on & _grow(~on, 1))
    pick = edge[rng.random(edge.size) < flying]
    z = f.ravel()[pick].astype(np.int64)
    t = rng.uniform(0.2, 0.8, size=pick.size)
    out.ravel()[pick] = np.clip(z + np.rint(t * (int(background) - z)), 1, 65535).astype(np.uint16)
    free = np.flatnonzero(_grow(on, int(ring)) & ~_grow(on, 1))
    spots = rng.choice(free, size=min(int(speckle), free.size), replace=False)
    mid = int(np.median(f[on]))
    out.ravel()[spots] = np.clip(mid + rng.integers(-int(jitter), int(jitter) + 1, size=spots.size),
                                 1, 65535).astype(np.uint16)
    return out


def rig_scene(hand_mm, wrist_cm, focal: float = 241.42, wall_mm: float = 800.0,
              arm_behind_cm: float = 1.0, arm_half_cm: float = 2.5, speckle: int = 15,
              speckle_mm: float = 150.0, seed: int = 0) -> np.ndarray:
    """What a camera of a rig sees around a rendered hand (240x320 float32 mm, 0 background): a
    wall at wall_mm behind everything, a forearm band from the wrist (camera coordinates, cm: a
    pose's theta 3..5) down to the bottom edge, arm_behind_cm behind the wrist and 2 *
    arm_half_cm wide, and `speckle` single pixels at speckle_mm scattered over the background
    (seeded).  The hand's own pixels stay as rendered: the input of the lane location's tests
    and bench."""
    hand = np.asarray(hand_mm, dtype=np.float32).reshape(240, 320)
    on = hand > 0
    out = np.where(on, hand, np.float32(wall_mm)).astype(np.float32)
    x, y, z = (float(v) for v in wrist_cm)
    col, row = 160.0 + focal * x / z, 120.0 + focal * y / z
    half = focal * arm_half_cm / (z + arm_behind_cm)
    r = np.arange(240)[:, None]
    c = np.arange(320)[None, :]
    arm = (r >= row) & (np.abs(c - col) <= half) & ~on
    out[arm] = np.float32((z + arm_behind_cm) * 10.0)
    free = np.flatnonzero(~on & ~arm)
    rng = np.random.default_rng(seed)
    out.ravel()[rng.choice(free, size=speckle, replace=False)] = np.float32(speckle_mm)
    return out
