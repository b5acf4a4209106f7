"""Float64 statement of the closed-loop re-aim (csrc/retarget.hip) and the table of cases the device is checked at.

NumPy on the host.  reaim64 is the formula of 5.2m, operation by operation, on the float32 inputs the kernel receives (sources,
targets and voxel are floats there; every one is widened to double first).  touched_sets builds the two bits of the `touched`
bitmaps and the mask count from first principles for any set of targets: bit 0 is the reference's rounded-texel sets
(drag_utils.py:322-334: the float32 lattice p + fl(voxel * k), th.round((p + 1) * (W - 1) / 2) in float32, the cast to int16, the
points outside the map dropped), bit 1 the 4x4 footprint around the bilinear corner floor(((double)u + 1) / 2 * (W - 1)) of
every TARGET lattice position.  A retarget must leave `touched` / `nmask` as touched_sets(sources, goals) gives them.

tests/test_retarget_ref_host.py pins the oracle and asserts the input conditions of every case; tests/test_gpu_retarget.py runs
the cases on the device.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

from tests import drag_ref as R

PLANE_AXES = ((0, 1), (1, 2), (0, 2))        # (column axis, row axis) of planes xy, yz, xz: csrc/drag.h plane_axes
LDS_BYTES = 65536                            # csrc/retarget.h RETARGET_LDS_BYTES: 3 * W * W may not exceed it
MARGIN = 1e-9                                # no d of a case lies this close to its step or arrive (d == 0 excepted)


# ------------------------------------------------------------------------------------------------ the re-aim
def reaim64(sources, targets, K, voxel, step, arrive):
    """DESIGN.md 5.2m for the handles of one edit.  sources, targets [B, 3] (taken as float32), K int [B, 3], voxel (taken as
    float32), step > 0 (may be inf), arrive >= 0 -> goals float32 [B, 3], remaining float32 [B], arrived bool [B], done bool,
    d float64 [B], hold bool [B] (the d <= step branch: goal is the target, a bit copy), goals64 float64 [B, 3] (the other
    branch before its one rounding to float; nan where d == 0)."""
    s32, t32 = np.asarray(sources, np.float32).reshape(-1, 3), np.asarray(targets, np.float32).reshape(-1, 3)
    s, t, k = s32.astype(np.float64), t32.astype(np.float64), np.asarray(K).reshape(-1, 3).astype(np.float64)
    vx, step = np.float64(np.float32(voxel)), np.float64(step)
    rem = (t - s) / vx - k
    d = np.sqrt((rem[:, 0] * rem[:, 0] + rem[:, 1] * rem[:, 1]) + rem[:, 2] * rem[:, 2])
    hold = d <= step
    with np.errstate(invalid="ignore", divide="ignore"):
        g64 = s + vx * (k + step * rem / d[:, None])
    goals = np.where(hold[:, None], t32, g64.astype(np.float32)).astype(np.float32)
    arrived = d <= np.float64(arrive)
    return SimpleNamespace(goals=goals, remaining=d.astype(np.float32), arrived=arrived, done=bool(arrived.all()), d=d, hold=hold,
                           goals64=g64)


def ulps32(a, b):
    """Distance in float32 units in the last place between two float32 arrays of finite values (0: the same bits or +-0)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------ the touched sets
def lattice32(p, voxel, r):
    """float32 [len(p), 2r+1]: p + fl(voxel * k), k = -r..r (csrc/drag.h lattice; drag_utils.py:314-316)."""
    k = np.arange(-r, r + 1, dtype=np.float32)
    return (np.asarray(p, np.float32)[:, None] + (np.float32(voxel) * k)[None, :]).astype(np.float32)


def _round_texel(u, W):
    """th.round((u + 1) * (W - 1) / 2).type(int16) in float32, as a Python int array."""
    x = np.rint(((u + np.float32(1)) * np.float32(W - 1)) / np.float32(2)).astype(np.int64)
    return ((x + 32768) % 65536) - 32768


def touched_sets(sources, targets, r, voxel, W):
    """uint8 [3, W, W] (indexed [plane][row][col]) with bit 0 and bit 1 as the module docstring defines them, and nmask, the
    number of texels with bit 0 clear."""
    out = np.zeros((3, W, W), np.uint8)
    src, tgt = np.asarray(sources, np.float32).reshape(-1, 3), np.asarray(targets, np.float32).reshape(-1, 3)
    for p, (ac, ar) in enumerate(PLANE_AXES):
        for pts, is_target in ((src, False), (tgt, True)):
            for b in range(len(pts)):
                u, v = lattice32(pts[b:b + 1, ac], voxel, r)[0], lattice32(pts[b:b + 1, ar], voxel, r)[0]
                for col in _round_texel(u, W):
                    for row in _round_texel(v, W):
                        if 0 <= col < W and 0 <= row < W:
                            out[p, row, col] |= 1
                if is_target:
                    x0 = np.floor((u.astype(np.float64) + 1.0) / 2.0 * (W - 1)).astype(np.int64)
                    y0 = np.floor((v.astype(np.float64) + 1.0) / 2.0 * (W - 1)).astype(np.int64)
                    for x in x0:
                        for y in y0:
                            c0, c1, r0, r1 = max(x - 1, 0), min(x + 2, W - 1), max(y - 1, 0), min(y + 2, W - 1)
                            if c0 <= c1 and r0 <= r1:
                                out[p, r0:r1 + 1, c0:c1 + 1] |= 2
    return out, int(((out & 1) == 0).sum())


# ------------------------------------------------------------------------------------------------ the cases
_F_SRC, _F_TGT = R._F_SRC, R._F_TGT
_INF = float("inf")


def _on_lattice(src, voxel, k):
    """source + voxel * k where that is exact in float32 (the caller's choice of numbers), so T = k exactly."""
    return (np.asarray(src, np.float32) + np.float32(voxel) * np.asarray(k, np.float32)).astype(np.float32)


def _case_K():
    v = 2 / 32
    src = np.array([[0.30, -0.21, 0.12], [-0.41, 0.17, 0.33], [0.25, -0.5, 0.125]], np.float32)
    # handle 0: T ~ (2.3, -1.2, 0.7), K overshoots it: d ~ 1.1 <= step; handle 1: T ~ (5.4, -3.3, 2.2), K on the far side of the
    # source: d ~ 7.9 > step; handle 2: the target is source + voxel * K exactly (all dyadic): d == 0
    tgt = np.stack([src[0] + np.float32(v) * np.array([2.3, -1.2, 0.7], np.float32),
                    src[1] + np.float32(v) * np.array([5.4, -3.3, 2.2], np.float32),
                    _on_lattice(src[2], v, [3, -2, 1])]).astype(np.float32)
    return [src], [tgt], [np.array([[3, -2, 1], [-1, 1, 4], [3, -2, 1]], np.int32)]


def _case_F():
    # K = round(T) for handles 0 and 3, whose targets have the coordinates 1 and -1.05: they are within the lead, so their GOALS
    # are those targets, at and beyond the map's edge, as a column and as a row of some plane; handles 1 and 2 aim from K = 0 at
    # targets far outside (and handle 2 starts outside)
    T = (_F_TGT.astype(np.float64) - _F_SRC.astype(np.float64)) / np.float64(np.float32(0.2))
    K = np.rint(T).astype(np.int32)
    K[1] = 0
    K[2] = 0
    return [_F_SRC], [_F_TGT], [K]


def _random(seed, counts, spread=0.6, move=0.5, kmax=3):
    gen = torch.Generator().manual_seed(seed)
    src, tgt, K = [], [], []
    for n in counts:
        s, t = R._handles(gen, n, spread=spread, move=move)
        src.append(np.ascontiguousarray(s, np.float32))
        tgt.append(np.ascontiguousarray(t, np.float32))
        K.append(torch.randint(-kmax, kmax + 1, (n, 3), generator=gen).numpy().astype(np.int32))
    return src, tgt, K


def _case_A():
    s, t, K = _random(301, (2,))
    return s, t, [np.zeros_like(K[0])]


def _case_L():
    s, t, K = _random(303, (1, 3, 2))
    v = np.float64(np.float32(2 / 32))
    K[0] = np.rint((t[0].astype(np.float64) - s[0].astype(np.float64)) / v).astype(np.int32)      # edit 0 has arrived: done
    return s, t, K


def _case_J():
    s, t, K = _random(304, (3,), spread=0.5, move=0.3, kmax=6)
    return s, t, K


#        W   ld   chmap                        r   voxel    handles            step  arrive  tap seed
_TABLE = {
    "A": (16, 32, lambda: R._arange_map(8), 2, 2 / 32, _case_A, 1.5, 1.0, 401),
    "K": (16, 32, lambda: R._arange_map(8), 2, 2 / 32, _case_K, 1.5, 1.0, 402),
    "F": (24, 32, lambda: R._arange_map(8), 2, 0.2, _case_F, 3.0, 0.75, 403),
    "L": (16, 32, lambda: R._arange_map(8), 2, 2 / 32, _case_L, 1.5, 2.0, 404),
    "J": (64, 512, lambda: R._product_map(512), 12, 2 / 256, _case_J, 2.0, 1.0, None),          # the real shape, once
    "INF": (16, 32, lambda: R._arange_map(8), 2, 2 / 32, _case_A, _INF, 1.0, 401),
}
CASES = tuple(_TABLE)
LOSS_CASES = ("A", "F", "L")                 # the cases whose taps are made (the loss after a retarget)


@lru_cache(maxsize=None)
def make_case(name):
    W, ld, chmap, r, voxel, handles, step, arrive, seed = _TABLE[name]
    sources, targets, K = handles()
    counts = [len(s) for s in sources]
    offs = np.concatenate(([0], np.cumsum(counts))).astype(int).tolist()
    chmap = np.ascontiguousarray(chmap(), dtype=np.int32)
    edits = origs = None
    if seed is not None:
        gen = torch.Generator().manual_seed(seed)
        taps = [R._taps(gen, W, ld, 1.0) for _ in counts]
        edits, origs = torch.stack([t[0] for t in taps]), torch.stack([t[1] for t in taps])
    return SimpleNamespace(name=name, W=W, ld=ld, chmap=chmap, Cc=chmap.shape[1], r=r, voxel=voxel, E=len(counts), sources=sources,
                           targets=targets, K=K, offsets=offs, step=step, arrive=arrive, edits=edits, origs=origs)


@lru_cache(maxsize=None)
def oracle(name):
    """Per edit: reaim64 of the case plus touched / nmask of touched_sets(sources, goals).  Computed once per session and shared;
    callers do not modify it."""
    c = make_case(name)
    out = []
    for e in range(c.E):
        o = reaim64(c.sources[e], c.targets[e], c.K[e], c.voxel, c.step, c.arrive)
        o.touched, o.nmask = touched_sets(c.sources[e], o.goals, c.r, c.voxel, c.W)
        out.append(o)
    return out
