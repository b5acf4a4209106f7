"""Float64 oracle of the drag loss (csrc/drag.hip) and the table of cases the device is checked at.

Plain torch on the CPU, no device code.  The oracle takes the tap as the kernel sees it ([W*W, ld], fp16 values), gathers
[3, Cc, W, W] through the channel map, computes the reference's loss (drag_utils.py:355-382, as oracle/ref_cpu.py::drag_loss
does) in float64 with the bilinear sampling written out (four corners, align_corners=True, zeros padding) and returns the loss
and d loss / d tap in the tap's own layout by autograd back through the gather: repeated channels sum, unmapped and padding
channels get exactly 0.  The lattice coordinates and the mask sets are the reference's own float32 ones (O.DragSetup), cast to
float64: the oracle samples where the reference samples, not at better coordinates.

tests/test_drag_ref_host.py pins the oracle (G7 golden, F.grid_sample) and asserts the input conditions of every case;
tests/test_gpu_drag_oracle.py runs the cases on the device.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

DSEG = 5                    # csrc/drag.hip: consecutive lattice positions a wave walks
TIE_MARGIN = 1e-4           # no texel coordinate of a case's lattices is this close to a half-integer
L1_AMBIGUOUS = 1e-5         # |d64| below this times max|feature| (and not 0): fp32 and fp64 may disagree on the sign
L1_EXCLUDED_CAP = 0.01      # share of the non-zero elements of g64 the L1 comparison may leave out


# ------------------------------------------------------------------------------------------------ the oracle
def gather_planes(tap, chmap, W):
    """tap [W*W, ld] -> [3, Cc, W, W]: plane p, channel c is tap channel chmap[p][c] (resize_feat_align as a gather)."""
    cm = torch.as_tensor(np.asarray(chmap), dtype=torch.long).reshape(3, -1)
    return tap[:, cm.reshape(-1)].t().reshape(3, cm.shape[1], W, W)


def corners(grid, W):
    """grid [..., 2] (normalised, [..., 0] indexes columns) -> texel coordinates ix, iy and their floors, align_corners=True."""
    ix = (grid[..., 0] + 1) / 2 * (W - 1)
    iy = (grid[..., 1] + 1) / 2 * (W - 1)
    return ix, iy, torch.floor(ix), torch.floor(iy)


def sample_bilinear(feat, grid):
    """feat [P, C, W, W], grid [P, B, N, 2] -> [P, C, B, N]; bilinear, zeros padding, align_corners=True, in feat's dtype."""
    P, C, H, W = feat.shape
    assert H == W
    _, B, N, _ = grid.shape
    ix, iy, x0, y0 = corners(grid, W)
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = 1 - wx1, 1 - wy1
    flat = feat.reshape(P, C, H * W)
    out = 0
    for dy, dx, w in ((0, 0, wx0 * wy0), (0, 1, wx1 * wy0), (1, 0, wx0 * wy1), (1, 1, wx1 * wy1)):
        x, y = x0 + dx, y0 + dy
        inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        idx = (y.clamp(0, H - 1) * W + x.clamp(0, W - 1)).long().reshape(P, 1, B * N).expand(P, C, B * N)
        v = torch.gather(flat, 2, idx).reshape(P, C, B, N)
        out = out + v * (w * inside).unsqueeze(1)
    return out


def _loss(fe, fo, setup, cof, loss_type, sampler):
    patch = sampler(fo, setup.patch_grid.to(fo.dtype))
    shift = sampler(fe, setup.shift_grid.to(fe.dtype))
    d = shift - patch.detach()
    motion = d.abs().mean() if loss_type == "l1" else (d ** 2).mean()
    nmask = sum(int(m.sum()) for m in setup.masks)
    mask_term = torch.zeros((), dtype=fe.dtype)
    if cof > 0:
        tot = 0
        for p in range(3):
            dm = (fe[p] - fo[p])[:, setup.masks[p]]
            tot = tot + (dm.abs().sum() if loss_type == "l1" else (dm ** 2).sum())
        mask_term = tot / (fe.shape[1] * nmask)
    return -motion - cof * mask_term, d.detach(), nmask


def drag_loss_grad64(edit_tap, orig_tap, chmap, sources, targets, r, voxel, W, cof, loss_type, sampler=sample_bilinear):
    """The float64 loss and gradient.  Returns loss (float), grad [W*W, ld] float64, d [3, Cc, B, (2r+1)^3] (the sample
    differences shift - patch), setup (O.DragSetup: float32 grids, mask sets) and nmask."""
    setup = O.DragSetup(sources, targets, r, voxel, W)
    cof = float(np.float32(cof))            # the kernels take cof as a C float
    e = edit_tap.detach().double().requires_grad_(True)
    fe, fo = gather_planes(e, chmap, W), gather_planes(orig_tap.detach().double(), chmap, W)
    loss, d, nmask = _loss(fe, fo, setup, cof, loss_type, sampler)
    grad, = torch.autograd.grad(loss, e)
    return SimpleNamespace(loss=float(loss.detach()), grad=grad, d=d, setup=setup, nmask=nmask)


def grid_sample64(feat, grid):
    return F.grid_sample(feat, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def drag_loss_grad32(edit_tap, orig_tap, chmap, sources, targets, r, voxel, W, cof, loss_type):
    """The reference's own float32 arithmetic on the same inputs (O.drag_loss, autograd), gathered the same way: the yardstick
    the device's error is measured in."""
    setup = O.DragSetup(sources, targets, r, voxel, W)
    cof = float(np.float32(cof))
    e = edit_tap.detach().float().requires_grad_(True)
    loss = O.drag_loss(gather_planes(e, chmap, W), gather_planes(orig_tap.detach().float(), chmap, W), setup, cof, loss_type)
    grad, = torch.autograd.grad(loss, e)
    return float(loss.detach()), grad


def l1_ambiguous_elements(res, edit_tap, orig_tap, chmap, W):
    """bool [W*W, ld]: tap elements in the 2x2 target footprint of a sample whose difference is not 0 but below L1_AMBIGUOUS *
    max|feature| -- the L1 gradient there depends on a sign the two precisions can disagree on."""
    cm = np.asarray(chmap).reshape(3, -1)
    thr = L1_AMBIGUOUS * max(float(edit_tap.abs().max()), float(orig_tap.abs().max()))
    out = torch.zeros(edit_tap.shape, dtype=torch.bool)
    a = res.d.abs()
    _, _, x0, y0 = corners(res.setup.shift_grid.double(), W)
    for p, c, b, n in torch.nonzero((a > 0) & (a < thr)).tolist():
        for dy in (0, 1):
            for dx in (0, 1):
                x, y = int(x0[p, b, n]) + dx, int(y0[p, b, n]) + dy
                if 0 <= x < W and 0 <= y < W:
                    out[y * W + x, cm[p, c]] = True
    return out


# ------------------------------------------------------------------------------------------------ loss scale
def pick_scale_ref(m):
    """The power-of-two loss scale of max|g| = m: 2^floor(log2(256 / m)) within [2^-20, 2^99]; 1 for 0, inf and nan."""
    m = float(np.float32(m))
    sc = 1.0
    if m > 0 and np.isfinite(m):
        sc = 2.0 ** np.floor(np.log2(256.0 / m))
    return np.float32(min(max(sc, 2.0 ** -20), 2.0 ** 99))


def scaled_f16_ref(g, sc):
    """fp16(g * sc): the product in float32, then numpy's round-to-nearest-even cast."""
    with np.errstate(over="ignore"):
        return (np.asarray(g, np.float32) * np.float32(sc)).astype(np.float16)


# ------------------------------------------------------------------------------------------------ the launcher's grids, restated
def terms_blocks(B, r, Cc):
    side = 2 * r + 1
    rows = 3 * B * side * ((Cc + 63) // 64) * ((side + DSEG - 1) // DSEG)
    return min((rows * 64 + 255) // 256, 1024)


def gather_blocks(W, ld):
    return min((W * W * ld // 8 + 255) // 256, 512)


# ------------------------------------------------------------------------------------------------ the cases
def _arange_map(Cc):
    return np.arange(3 * Cc, dtype=np.int32).reshape(3, Cc)


def _product_map(channels):
    from ishapediting_amd.drag_utils import feat_channel_map
    return feat_channel_map(channels)


# one tap channel used twice within a plane (3), one used by two planes (5), the rest of the 32 unused
_H_MAP = np.array([[3, 3, 5, 7, 9, 11], [5, 12, 13, 14, 15, 16], [20, 21, 22, 23, 24, 25]], np.int32)

# F: ix = 7.5 (u + 1) + 0.46875 k, k = -2..2.  u = 1 gives 14.06 .. 15 (exactly W-1) .. 15.94 (x0 = W-1, x1 outside);
# u = -1.05 gives -1.31 (wholly outside) .. -0.84, -0.375 (x0 = -1) .. 0.56; handle 1's target is outside on every plane,
# handle 2's source is.  Each coordinate appears as a column and as a row of some plane.
_F_SRC = np.array([[-1.05, 0.2, 1.0], [0.5, -0.3, 0.1], [-1.7, 1.5, 1.5], [1.0, -1.05, 0.2]], np.float32)
_F_TGT = np.array([[1.0, -1.05, 0.3], [1.5, 1.5, -1.7], [-0.42, 0.6, -0.6], [-1.05, 0.3, 1.0]], np.float32)

#        W   ld   chmap                       r   voxel     handles  seed  feature scale
_TABLE = {
    "A": (16, 64, lambda: _arange_map(20), 2, 2 / 32, 2, 101, 1.0),
    "B": (16, 224, lambda: _arange_map(70), 3, 2 / 32, 2, 102, 1.0),
    "C": (16, 192, lambda: _arange_map(64), 0, 2 / 32, 3, 103, 1.0),
    "D": (24, 32, lambda: _arange_map(8), 1, 0.2, 3, 104, 1.0),
    "E": (16, 32, lambda: _arange_map(8), 2, 2 / 15, 1, 105, 1.0),
    "F": (16, 64, lambda: _arange_map(20), 2, 2 / 32, "F", 106, 1.0),
    "G": (16, 64, lambda: _product_map(64), 2, 2 / 32, 2, 107, 1.0),
    "H": (16, 32, lambda: _H_MAP, 2, 2 / 32, 2, 108, 1.0),
    "I": (16, 64, lambda: _arange_map(20), 2, 2 / 32, "I", 109, 1.0),
    "J": (64, 512, lambda: _product_map(512), 12, 2 / 128, 1, 110, 1.0),
    "K6": (16, 224, lambda: _arange_map(70), 3, 2 / 32, 2, 102, 2.0 ** -6),
    "K12": (16, 224, lambda: _arange_map(70), 3, 2 / 32, 2, 102, 2.0 ** -12),
}
CASES = tuple(_TABLE)
# J runs once per loss type; every other case for l2 / l1 x cof 0 / 0.4
COMBOS = tuple((c, lt, cof) for c in CASES for lt in ("l2", "l1") for cof in (0.0, 0.4)
               if c != "J" or (lt, cof) in (("l2", 0.4), ("l1", 0.0)))


def _taps(gen, W, ld, scale):
    """randn features rounded to fp16 (every tap channel, mapped or not), orig = edit + 0.3 randn."""
    e = torch.randn(W * W, ld, generator=gen)
    o = e + 0.3 * torch.randn(W * W, ld, generator=gen)
    return (e * scale).half(), (o * scale).half()


def _handles(gen, n, spread=0.8, move=0.4):
    s = torch.rand(n, 3, generator=gen) * 2 * spread - spread
    t = s + (torch.rand(n, 3, generator=gen) - 0.5) * move
    return s.numpy(), t.numpy()


@lru_cache(maxsize=None)
def make_case(name):
    W, ld, chmap, r, voxel, handles, seed, scale = _TABLE[name]
    gen = torch.Generator().manual_seed(seed)
    edit, orig = _taps(gen, W, ld, scale)
    if handles == "F":
        src, tgt = _F_SRC, _F_TGT
    elif handles == "I":          # handles 0 and 1 share a target, handle 2 does not move
        src, tgt = _handles(gen, 4)
        tgt[1] = tgt[0]
        tgt[2] = src[2]
    elif name == "D":
        # ix = 11.5 (u + 1) + 2.3 k, k = -1..1.  Sources anywhere in +-1.0; every target coordinate sits (with a drawn jitter of
        # +-0.02) where its lattice leaves the map: |u| = 0.85 puts the outer position partly outside (ix in (-1, 0) or
        # (W-1, W)), |u| = 0.95 wholly outside.  Each of the four occurs among the column and among the row coordinates.
        src, _ = _handles(gen, handles, spread=1.0)
        tgt = np.array([[-0.85, 0.85, -0.95], [0.95, -0.95, 0.85], [0.3, -0.85, 0.95]], np.float32)
        tgt = tgt + ((torch.rand(3, 3, generator=gen) - 0.5) * 0.04).numpy()
    else:
        src, tgt = _handles(gen, handles)
    chmap = np.ascontiguousarray(chmap(), dtype=np.int32)
    return SimpleNamespace(name=name, W=W, ld=ld, chmap=chmap, Cc=chmap.shape[1], r=r, voxel=voxel, side=2 * r + 1,
                           sources=np.ascontiguousarray(src, np.float32), targets=np.ascontiguousarray(tgt, np.float32),
                           B=len(src), edit=edit, orig=orig)


@lru_cache(maxsize=None)
def make_batch():
    """L: E = 3 edits of case B's tap shape with 1, 3 and 2 handles and cof 0 / 0.2 / 0.4; one guidance tap per edit (the shared
    form reads the first)."""
    b = make_case("B")
    gen = torch.Generator().manual_seed(111)
    taps = [_taps(gen, b.W, b.ld, 1.0) for _ in range(3)]
    hs = [_handles(gen, n) for n in (1, 3, 2)]
    return SimpleNamespace(W=b.W, ld=b.ld, chmap=b.chmap, Cc=b.Cc, r=b.r, voxel=b.voxel, side=b.side, E=3,
                           cofs=(0.0, 0.2, 0.4), edits=torch.stack([t[0] for t in taps]), origs=torch.stack([t[1] for t in taps]),
                           sources=[h[0] for h in hs], targets=[h[1] for h in hs])


@lru_cache(maxsize=None)
def oracle(name, loss_type, cof):
    """drag_loss_grad64 of a case, computed once per session and shared; callers do not modify it."""
    c = make_case(name)
    return drag_loss_grad64(c.edit, c.orig, c.chmap, c.sources, c.targets, c.r, c.voxel, c.W, cof, loss_type)


@lru_cache(maxsize=None)
def reference32(name, loss_type, cof):
    c = make_case(name)
    return drag_loss_grad32(c.edit, c.orig, c.chmap, c.sources, c.targets, c.r, c.voxel, c.W, cof, loss_type)


@lru_cache(maxsize=None)
def oracle_batch(loss_type, shared):
    L = make_batch()
    out = []
    for e in range(L.E):
        o = L.origs[0 if shared else e]
        a = (L.edits[e], o, L.chmap, L.sources[e], L.targets[e], L.r, L.voxel, L.W, L.cofs[e], loss_type)
        out.append((drag_loss_grad64(*a), drag_loss_grad32(*a)))
    return out


# ------------------------------------------------------------------------------------------------ coverage witnesses
def texel_coords(setup, W):
    """Every texel coordinate (u + 1) (W - 1) / 2 of the source and target lattices, float64 of the float32 lattice."""
    g = torch.cat((setup.patch_grid.reshape(-1), setup.shift_grid.reshape(-1))).double()
    return (g + 1) * (W - 1) / 2


def tie_margin(setup, W):
    """Distance of the closest lattice texel coordinate to a half-integer (where round() of the mask sets would be ambiguous)."""
    t = texel_coords(setup, W)
    return float(((t - torch.floor(t)) - 0.5).abs().min())


def walk_columns(setup, c):
    """floor(ix) of the target along each lattice row the motion kernel walks: int64 [3, B, side] (the column coordinate of
    plane p depends only on the lattice index along its column axis)."""
    side, B = c.side, c.B
    g = setup.shift_grid.double().reshape(3, B, side, side, side, 2)
    cols = torch.stack((g[0, :, :, 0, 0, 0], g[1, :, 0, :, 0, 0], g[2, :, :, 0, 0, 0]))       # planes xy, yz, xz: columns x, y, x
    return torch.floor((cols + 1) / 2 * (c.W - 1)).long()


def tail_positions(side):
    """(live, dead) positions of the last segment of a lattice row when it is not a full one, else None."""
    live = side % DSEG
    return (live, DSEG - live) if side > DSEG and live else None
