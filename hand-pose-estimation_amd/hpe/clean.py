"""Host mirror of lane cleaning (hpe_set_batch_clean, include/hpe.h "Lane cleaning"): the
neighbourhood rule on a 240x320 uint16 frame, in plain numpy, for callers that clean frames
themselves and for the tests.

F is the frame, and the eight neighbours q of pixel p read 0 outside the image.  With u = F[p]:
    near(q)  <=>  F[q] != 0 and |F[q] - u| <= edge
    s = the number of near neighbours
    out[p] = 0                   if u == 0 or s < support
           = sorted(C)[s // 2]   with the median, C = {u} + {F[q] : near(q)}
           = u                   otherwise
Integers only: the device's result is this one, bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

IMG_H, IMG_W = 240, 320
MEDIAN = 1  # HPE_CLEAN_MEDIAN
FIELDS = ("edge", "support", "flags", "pad")
# the eight neighbours' offsets {row, column}
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def clean(frame_u16, edge, support, median):
    """The rule on one uint16 frame (any 2-D shape; the device's is 240x320): a new uint16
    array.  Nothing is converted silently."""
    f = np.asarray(frame_u16)
    if f.dtype != np.uint16 or f.ndim != 2:
        raise TypeError(f"clean takes 2-D uint16 frames, got {f.dtype} with {f.ndim} axes")
    edge, support = int(edge), int(support)
    if not 0 <= edge <= 65535 or not 0 <= support <= 8:
        raise ValueError(f"edge {edge} outside 0..65535 or support {support} outside 0..8")
    h, w = f.shape
    pad = np.zeros((h + 2, w + 2), dtype=np.int32)
    pad[1:-1, 1:-1] = f
    u = pad[1:-1, 1:-1]
    nb = np.stack([pad[1 + dr:1 + dr + h, 1 + dc:1 + dc + w] for dr, dc in NEIGHBOURS])
    near = (nb != 0) & (np.abs(nb - u[None]) <= edge)
    s = near.sum(axis=0)
    out = u.copy()
    if median:
        big = np.int32(1 << 20)  # sorts behind every 16-bit value
        c = np.concatenate([u[None], np.where(near, nb, big)])
        c.sort(axis=0)
        out = np.take_along_axis(c, (s // 2)[None], axis=0)[0]
    return np.where((u != 0) & (s >= support), out, 0).astype(np.uint16)


@dataclass(frozen=True)
class Clean:
    """hpe_clean: one lane's parameters."""
    edge: int
    support: int
    flags: int = 0
    pad: int = 0

    def __post_init__(self):
        for f in FIELDS:
            object.__setattr__(self, f, int(getattr(self, f)))

    @property
    def median(self) -> bool:
        return bool(self.flags & MEDIAN)

    def check(self) -> "Clean":
        """The library's refusals (HPE_E_ARG there, ValueError here); returns self."""
        if not 0 <= self.edge <= 65535:
            raise ValueError(f"clean edge {self.edge} outside 0..65535")
        if not 0 <= self.support <= 8:
            raise ValueError(f"clean support {self.support} outside 0..8")
        if self.flags & ~MEDIAN or self.pad:
            raise ValueError(f"unknown clean flags {self.flags:#x} or non-zero pad {self.pad}")
        return self

    def apply(self, frame_u16):
        return clean(frame_u16, self.edge, self.support, self.median)


def defaults(unit_mm: float = 1.0) -> Clean:
    """hpe_clean_defaults: edge = lrint(15 / unit_mm) within 1..65535, support 3, the median.
    Untuned; tried on rendered scenes with synth.camera_noise only."""
    unit_mm = float(np.float32(unit_mm))
    if not (np.isfinite(unit_mm) and unit_mm > 0):
        raise ValueError(f"depth unit {unit_mm} mm is not finite and positive")
    e = float(np.rint(np.float64(15.0) / np.float64(unit_mm)))
    return Clean(int(min(max(e, 1.0), 65535.0)), 3, MEDIAN)


def as_clean(p) -> Clean:
    """A Clean, an object with the four fields (hpe._lib.CleanPar) or a sequence {edge, support
    [, flags [, pad]]} as a Clean."""
    if isinstance(p, Clean):
        return p
    if all(hasattr(p, f) for f in FIELDS):
        return Clean(*[getattr(p, f) for f in FIELDS])
    return Clean(*p)
