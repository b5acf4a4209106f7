"""Float64 oracle of the handle tracker (csrc/track.hip) and the table of cases the device is checked at.

Plain torch on the CPU.  The taps are the kernel's ([W*W, ld], fp16 values); planes are gathered through the channel map and
sampled with tests/drag_ref.py's gather_planes / sample_bilinear (four corners, align_corners=True, zeros padding) in float64,
at the float32 lattice coordinates the kernel forms: lattice(source, voxel, m) = source + fl(voxel * m) with the integer m summed
first (source side m = i, candidate side m = K_in + k + i).  D(b; k) is formed for every candidate by brute force from the
definition; the oracle also returns M(b; k) = sum(|shift| + |patch|), the scale the device's rounding error is measured in, and
the winner under the tie rule (smallest D, then smallest |k|^2, then lowest linear index).

tests/test_track_ref_host.py pins the oracle and asserts the input conditions of every case; tests/test_gpu_track.py runs the
cases on the device.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

from tests import drag_ref as R

PLANE_AXES = ((0, 1), (1, 2), (0, 2))        # (column axis, row axis) of planes xy, yz, xz: csrc/drag.h plane_axes
MAX_R, MAX_RP = 8, 4
LDS_BYTES = 65536                            # csrc/track.h TRACK_LDS_BYTES


# ------------------------------------------------------------------------------------------------ the launcher, restated
def chunk_width(Rs, rp):
    """Channels a workgroup stages at once: the widest of 64 / 32 / 16 whose fp32 samples fit LDS_BYTES."""
    n = (2 * (Rs + rp) + 1) ** 2 + (2 * rp + 1) ** 2
    for cw in (64, 32):
        if n * cw * 4 <= LDS_BYTES:
            return cw
    return 16


def scratch_bytes(E, Btot, Rs, rp, Cc):
    if not (1 <= E <= 32 and Btot >= E and Cc >= 1 and 0 <= Rs <= MAX_R and 0 <= rp <= MAX_RP):
        return -1
    cw = chunk_width(Rs, rp)
    return (Btot * 3 * ((Cc + cw - 1) // cw) * (2 * Rs + 1) ** 2 * 4 + 15) // 16 * 16


def chain_length(Rs, rp, Cc):
    """n, the additions of the kernel's longest chain behind one D: a lane adds ceil(P / nsub) patch terms in order
    (P = (2 rp + 1)^2 positions, nsub = 64 / chunk width lanes share a channel), 6 butterfly levels add the 64 lanes, the nchunk
    chunk sums are added in order, 2 additions join the three planes."""
    cw = chunk_width(Rs, rp)
    nsub, P = 64 // cw, (2 * rp + 1) ** 2
    return (P + nsub - 1) // nsub + 6 + (Cc + cw - 1) // cw + 2


def tolerance(M, Rs, rp, Cc):
    """The comparison tolerance: (n + 8) 2^-24 M.  The 8: per term, the two samples (weights rounded once, four
    fused multiply-adds each) and the subtraction, each at most one rounding relative to |shift| + |patch|."""
    return (chain_length(Rs, rp, Cc) + 8) * 2.0 ** -24 * M


# ------------------------------------------------------------------------------------------------ the oracle
def lattice32(s, voxel, m):
    """float32: the product rounded, then the sum (csrc/drag.h lattice)."""
    return (np.float32(s) + np.float32(voxel) * np.asarray(m, np.float32)).astype(np.float32)


def _sample_window(feat_p, W, ucol, vrow):
    """feat_p [C, W, W] float64 sampled at the grid rows vrow x columns ucol (float32 coordinates) -> [C, len(vrow), len(ucol)]."""
    g = torch.stack(torch.meshgrid(torch.from_numpy(vrow).double(), torch.from_numpy(ucol).double(), indexing="ij"), -1)
    grid = torch.stack((g[..., 1], g[..., 0]), -1).reshape(1, 1, -1, 2)          # [..., 0] indexes columns
    return R.sample_bilinear(feat_p[None], grid)[0, :, 0].reshape(feat_p.shape[0], len(vrow), len(ucol))


def plane_maps64(fe, fo, W, source, voxel, K, Rs, rp):
    """D_p and M_p of one handle: float64 [3, side (row offset), side (column offset)] each."""
    side, i = 2 * Rs + 1, np.arange(-rp, rp + 1)
    D, M = torch.zeros(3, side, side, dtype=torch.float64), torch.zeros(3, side, side, dtype=torch.float64)
    for p, (ac, ar) in enumerate(PLANE_AXES):
        patch = _sample_window(fo[p], W, lattice32(source[ac], voxel, i), lattice32(source[ar], voxel, i))
        for kr in range(-Rs, Rs + 1):
            for kc in range(-Rs, Rs + 1):
                shift = _sample_window(fe[p], W, lattice32(source[ac], voxel, int(K[ac]) + kc + i),
                                       lattice32(source[ar], voxel, int(K[ar]) + kr + i))
                D[p, kr + Rs, kc + Rs] = (shift - patch).abs().sum()
                M[p, kr + Rs, kc + Rs] = (shift.abs() + patch.abs()).sum()
    return D, M


def volume_of(maps, Rs):
    """[3, side, side] plane maps -> [side (kz), side (ky), side (kx)]: D_0(kx, ky) + D_1(ky, kz) + D_2(kx, kz)."""
    return maps[0][None, :, :] + maps[1][:, :, None] + maps[2][:, None, :]


def winner_of(vol, Rs):
    """The tie rule on a [side, side, side] volume -> ((kx, ky, kz), linear index, margin): margin is the runner-up's D minus
    the winner's (inf when there is one candidate)."""
    side = 2 * Rs + 1
    flat = vol.reshape(-1).double()
    k = torch.arange(side) - Rs
    r2 = (k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, :] ** 2).reshape(-1)
    ties = torch.nonzero(flat == flat.min()).reshape(-1)
    best = int(ties[torch.argmin(r2[ties] * side ** 3 + ties)])
    rest = torch.cat((flat[:best], flat[best + 1:]))
    margin = float(rest.min() - flat[best]) if len(rest) else float("inf")
    return (best % side - Rs, (best // side) % side - Rs, best // (side * side) - Rs), best, margin


def track64(edit_tap, orig_tap, chmap, W, sources, voxel, K_in, Rs, rp):
    """The oracle of one edit: D, M float64 [B, side^3] (linear index ((kz+R) side + ky+R) side + kx+R), winner int [B, 3]
    (k*, relative to K_in), index [B], margin [B]."""
    fe, fo = R.gather_planes(edit_tap.double(), chmap, W), R.gather_planes(orig_tap.double(), chmap, W)
    Ds, Ms, ks, idx, mar = [], [], [], [], []
    for b in range(len(sources)):
        D, M = plane_maps64(fe, fo, W, sources[b], voxel, K_in[b], Rs, rp)
        vol = volume_of(D, Rs)
        k, i, m = winner_of(vol, Rs)
        Ds.append(vol.reshape(-1)); Ms.append(volume_of(M, Rs).reshape(-1)); ks.append(k); idx.append(i); mar.append(m)
    return SimpleNamespace(D=torch.stack(Ds), M=torch.stack(Ms), winner=np.array(ks, np.int32), index=np.array(idx), margin=np.array(mar))


def brute_force_D(edit_tap, orig_tap, chmap, W, source, voxel, K, k, rp):
    """D(b; k) straight from the definition, one candidate, with no plane map in between (pins the separable form)."""
    fe, fo = R.gather_planes(edit_tap.double(), chmap, W), R.gather_planes(orig_tap.double(), chmap, W)
    i, tot = np.arange(-rp, rp + 1), 0.0
    for p, (ac, ar) in enumerate(PLANE_AXES):
        patch = _sample_window(fo[p], W, lattice32(source[ac], voxel, i), lattice32(source[ar], voxel, i))
        shift = _sample_window(fe[p], W, lattice32(source[ac], voxel, int(K[ac]) + k[ac] + i),
                               lattice32(source[ar], voxel, int(K[ar]) + k[ar] + i))
        tot += float((shift - patch).abs().sum())
    return tot


# ------------------------------------------------------------------------------------------------ the cases
# F: the coordinates of drag_ref._F_SRC at W 24, voxel 0.2: ix = 11.5 (u + 1) + 2.3 m, m up to +-(R + rp) = +-3.  u = 1 puts the
# window's far half outside on the right / bottom, u = -1.05 on the left / top, and each occurs as a column and as a row of some
# plane.  Handle 2's patch lies wholly outside on every plane, and so do the windows of k = 0 and of many other candidates: their D
# is exactly 0 and the tie rule decides (k* = 0).
_F_SRC = R._F_SRC

#        W   ld   chmap                         R  rp  voxel    handles per edit     K_in        seed  roll (rows, cols)
_TABLE = {
    "A": (16, 64, lambda: R._arange_map(20), 2, 1, 2 / 32, (2,), None, 201, (1, -1)),
    "B": (16, 224, lambda: R._arange_map(70), 3, 2, 2 / 32, (2,), None, 202, None),
    "C": (16, 192, lambda: R._arange_map(64), 0, 0, 2 / 32, (3,), None, 203, None),
    "E": (16, 32, lambda: R._arange_map(8), 1, 2, 2 / 15, (1,), None, 205, None),
    "F": (24, 32, lambda: R._arange_map(8), 2, 1, 0.2, "F", None, 206, None),
    "G": (16, 64, lambda: R._product_map(64), 2, 1, 2 / 32, (2,), None, 207, (-1, 1)),
    "H": (16, 32, lambda: R._H_MAP, 1, 1, 2 / 32, (2,), None, 208, None),
    "K": (16, 64, lambda: R._arange_map(20), 2, 1, 2 / 32, (2,), [[1, -2, 0], [-1, 1, 2]], 209, None),      # K_in + k crosses 0
    "L": (16, 224, lambda: R._arange_map(70), 2, 1, 2 / 32, (1, 3, 2), None, 211, None),                    # per-edit guidance
    "Ls": (16, 224, lambda: R._arange_map(70), 2, 1, 2 / 32, (1, 3, 2), None, 211, None),                   # shared guidance
    "P32": (16, 64, lambda: R._arange_map(20), 4, 4, 2 / 32, (1,), None, 212, None),                        # 32-channel chunks
    "P16": (16, 64, lambda: R._arange_map(20), 8, 4, 2 / 32, (1,), None, 213, None),                        # 16-channel chunks
    "J": (64, 512, lambda: R._product_map(512), 4, 2, 2 / 256, (1,), None, 210, None),                      # the real shape, once
}
CASES = tuple(_TABLE)
TIE_HANDLES = {"F": {(0, 2)}}          # (edit, handle) whose winning D = 0 is shared by several candidates, by construction


@lru_cache(maxsize=None)
def make_case(name):
    W, ld, chmap, Rs, rp, voxel, handles, K_in, seed, roll = _TABLE[name]
    gen = torch.Generator().manual_seed(seed)
    counts = (len(_F_SRC),) if handles == "F" else handles
    E = len(counts)
    taps = [R._taps(gen, W, ld, 1.0) for _ in range(E)]
    edits, origs = torch.stack([t[0] for t in taps]), torch.stack([t[1] for t in taps])
    if roll is not None:              # the edited tap is the guidance moved by whole texels plus noise: the winner is not k = 0
        edits = (torch.roll(origs.float().reshape(E, W, W, ld), roll, (1, 2)).reshape(E, W * W, ld) +
                 0.3 * torch.randn(E, W * W, ld, generator=gen)).half()
    if name == "Ls":
        origs = origs[:1]
    sources = [_F_SRC] if handles == "F" else [np.ascontiguousarray(R._handles(gen, n, spread=0.6)[0], np.float32) for n in counts]
    K = np.zeros((sum(counts), 3), np.int32) if K_in is None else np.asarray(K_in, np.int32)
    offs = np.concatenate(([0], np.cumsum(counts))).astype(int).tolist()
    chmap = np.ascontiguousarray(chmap(), dtype=np.int32)
    return SimpleNamespace(name=name, W=W, ld=ld, chmap=chmap, Cc=chmap.shape[1], R=Rs, rp=rp, voxel=voxel, side=2 * Rs + 1, E=E,
                           edits=edits, origs=origs, sources=sources, K_in=[K[offs[e]:offs[e + 1]] for e in range(E)], offsets=offs)


@lru_cache(maxsize=None)
def oracle(name):
    """track64 of every edit of a case, computed once per session and shared; callers do not modify it."""
    c = make_case(name)
    return [track64(c.edits[e], c.origs[e if c.origs.shape[0] > 1 else 0], c.chmap, c.W, c.sources[e], c.voxel, c.K_in[e], c.R, c.rp)
            for e in range(c.E)]


# ------------------------------------------------------------------------------------------------ the analytic case
def roll_case(k=(1, -2, 2), W=17, Cc=6, seed=214):
    """E is O with plane p's channels rolled by whole texels, k[column axis] columns and k[row axis] rows, at voxel = 2 / (W - 1)
    = 2^-3 and a source on a texel centre: every lattice coordinate is a texel centre exactly, in float32 and in float64, so the
    samples are the texels themselves, k* = k and D(k*) = 0 exactly.  The window stays inside the map (no wrap-around is read)."""
    gen = torch.Generator().manual_seed(seed)
    ld = 3 * Cc + 6
    chmap = R._arange_map(Cc)
    orig = torch.randn(W * W, ld, generator=gen).half()
    edit = orig.clone().reshape(W, W, ld)
    for p, (ac, ar) in enumerate(PLANE_AXES):
        ch = torch.as_tensor(chmap[p], dtype=torch.long)
        edit[:, :, ch] = torch.roll(orig.reshape(W, W, ld)[:, :, ch], (k[ar], k[ac]), (0, 1))
    return SimpleNamespace(W=W, ld=ld, chmap=chmap, Cc=Cc, R=2, rp=1, voxel=2.0 / (W - 1), k=k,
                           edit=edit.reshape(W * W, ld).contiguous(), orig=orig, sources=np.array([[0.0, 0.125, -0.125]], np.float32))
