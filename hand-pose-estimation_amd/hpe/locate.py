"""Host mirror of lane location (hpe_locate_depth, hpe_batch_pipeline_locate, include/hpe.h):
the location rule and the placement rule in plain numpy, for the tests and for callers that
locate on the host.

The location rule is the nearest-object heuristic of depth hand tracking: a histogram of the
valid pixels' quantised depth finds the nearest depth (past `skip` speckle pixels), the pixels
of a slab behind it give a first centre, and a fixed-size box around that centre gives the
second centre and the window.  Every fp64 value is computed from exact integer sums by one
written operation order, so the device result equals this mirror bit for bit.

`Params` is (search, bin, slab, half_xy, half_z, skip, min_pixels), `search` an
hpe.window.Window; `Result` mirrors hpe_locate without its seq and lane.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import window

IMG_H, IMG_W = 240, 320
K_BINS = 2048  # depth bins of the histogram; bin K_BINS - 1 takes everything beyond

Params = namedtuple("Params", ("search", "bin", "slab", "half_xy", "half_z", "skip", "min_pixels"))
Result = namedtuple("Result", ("found", "k_near", "m1", "m2", "px", "centre", "window"))
# hpe_locate_defaults: untuned values, tried on rendered scenes only
DEFAULTS = Params(window.WHOLE, 0.5, 12.0, 11.0, 11.0, 20, 200)
NO_WINDOW = window.Window(0, 0, 0, 0, 0.0, 0.0)  # the window of a result that is not found


def as_params(p) -> Params:
    p = Params(*p)
    return Params(window.as_window(p.search), float(p.bin), float(p.slab), float(p.half_xy),
                  float(p.half_z), int(p.skip), int(p.min_pixels))


def raw_values(depth, unit_mm=None):
    """The raw float frame: float32 pixels as they are, or float32(u) * float32(unit_mm) for
    uint16 pixels (the u16 batch's rule, one fp32 multiply)."""
    d = np.asarray(depth)
    if unit_mm is not None:
        if d.dtype != np.uint16:
            raise TypeError(f"a unit belongs to uint16 frames, got {d.dtype}")
        return (d.astype(np.float32) * np.float32(unit_mm)).reshape(IMG_H, IMG_W)
    if d.dtype == np.uint16:
        raise TypeError("uint16 frames need their unit_mm")
    return np.asarray(d, dtype=np.float32).reshape(IMG_H, IMG_W)


def _clamp_lo(v, lo, top):
    return int(min(max(v, float(lo)), float(top)))


def _clamp_hi(v, hi):
    return int(min(max(v, -1.0), float(hi)))


def box(r, c, z, focal, half_xy, half_z, search) -> window.Window:
    """The hand box around pixel (r, c) at depth z, clamped to the image and to `search`: each
    bound clamped in fp64 before its conversion to int, as the pose rule clamps."""
    s = window.as_window(search)
    hx = (float(focal) * float(half_xy)) / z
    zl, zh = z - half_z, z + half_z
    if s.z_lo > zl:
        zl = s.z_lo
    if s.z_hi < zh:
        zh = s.z_hi
    return window.Window(_clamp_lo(float(np.ceil(r - hx)), max(0, s.row_lo), IMG_H),
                         _clamp_hi(float(np.floor(r + hx)), min(IMG_H - 1, s.row_hi)),
                         _clamp_lo(float(np.ceil(c - hx)), max(0, s.col_lo), IMG_W),
                         _clamp_hi(float(np.floor(c + hx)), min(IMG_W - 1, s.col_hi)),
                         float(zl), float(zh))


def _centre(sel, rr, cc, k, bin_):
    m = int(sel.sum())
    sr, sc, sk = int(rr[sel].sum()), int(cc[sel].sum()), int(k[sel].sum())
    return m, float(sr) / float(m), float(sc) / float(m), (float(sk) / float(m) + 0.5) * bin_


def locate(depth, focal, params=DEFAULTS, to_cm=True, unit_mm=None) -> Result:
    """The location rule on one raw 240x320 frame (float mm, or uint16 with unit_mm)."""
    p = as_params(params)
    s = p.search
    focal = float(focal)
    rv = raw_values(depth, unit_mm)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Z = rv.astype(np.float64) / 10. if to_cm else rv.astype(np.float64)
        rr, cc = np.meshgrid(np.arange(IMG_H, dtype=np.int64), np.arange(IMG_W, dtype=np.int64),
                             indexing="ij")
        valid = (np.isfinite(rv) & (rv > 0) & (rr >= s.row_lo) & (rr <= s.row_hi) &
                 (cc >= s.col_lo) & (cc <= s.col_hi) & (Z >= s.z_lo) & (Z <= s.z_hi))
        kf = np.floor(np.where(valid, Z, 0.0) / p.bin)
    k = np.where(kf >= K_BINS - 1, K_BINS - 1, kf).astype(np.int64)
    hist = np.bincount(k[valid], minlength=K_BINS)
    over = np.nonzero(np.cumsum(hist) > p.skip)[0]
    none = Result(0, -1, 0, 0, (0.0, 0.0), (0.0, 0.0, 0.0), NO_WINDOW)
    if len(over) == 0:
        return none
    k_near = int(over[0])
    sb = int(min(float(np.ceil(p.slab / p.bin)), float(K_BINS)))
    m1, r1, c1, z1 = _centre(valid & (k >= k_near) & (k <= k_near + sb), rr, cc, k, p.bin)
    b1 = box(r1, c1, z1, focal, p.half_xy, p.half_z, s)
    in2 = (valid & (rr >= b1.row_lo) & (rr <= b1.row_hi) & (cc >= b1.col_lo) & (cc <= b1.col_hi) &
           (Z >= b1.z_lo) & (Z <= b1.z_hi))
    m2 = int(in2.sum())
    if m2 < p.min_pixels or m2 == 0:
        return none._replace(k_near=k_near, m1=m1, m2=m2)
    m2, r2, c2, z2 = _centre(in2, rr, cc, k, p.bin)
    centre = (((c2 - 160.0) * z2) / focal, ((r2 - 120.0) * z2) / focal, z2)
    return Result(1, k_near, m1, m2, (c2, r2), centre,
                  box(r2, c2, z2, focal, p.half_xy, p.half_z, s))


def centroid(S_cam):
    """The mean of the 48 centres in camera coordinates, summed in sphere order."""
    S = np.asarray(S_cam, dtype=np.float64).reshape(-1, 3)
    out = []
    for q in range(3):
        acc = 0.0
        for j in range(len(S)):
            acc = acc + float(S[j, q])
        out.append(acc / float(len(S)))
    return np.array(out)


def camera_centres(S):
    """hpe_build_spheres' centres (y and z negated) back in camera coordinates."""
    S = np.asarray(S, dtype=np.float64).reshape(-1, 3)
    return np.stack([S[:, 0], S[:, 1] * -1, S[:, 2] * -1], axis=1)


def place(S_cam, template, centre):
    """The placement rule: the 26-entry pose `template` with theta 3..5 moved so that the
    centroid of its sphere centres S_cam (camera coordinates, of the lane's hand at `template`)
    lands on `centre`."""
    row = np.array(template, dtype=np.float64).ravel()[:26].copy()
    cen = centroid(S_cam)
    for q in range(3):
        row[3 + q] = row[3 + q] + (float(centre[q]) - cen[q])
    return row
