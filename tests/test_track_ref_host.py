"""tests/track_ref.py pinned on the CPU (F.grid_sample in float64, an analytic whole-texel roll, the definition's brute force), the
input conditions of every tracking case, and the host side of ABI 21: symbols, the scratch-size formula, kernel metadata."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import drag_ref as R
from tests import track_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", ("A", "F", "K"))
def test_oracle_window_sampling_is_grid_sample_in_float64(name):
    """The plane maps recomputed with F.grid_sample (bilinear, zeros, align_corners=True) at the same float32 lattice."""
    c = K.make_case(name)
    fe, fo = R.gather_planes(c.edits[0].double(), c.chmap, c.W), R.gather_planes(c.origs[0].double(), c.chmap, c.W)
    i = np.arange(-c.rp, c.rp + 1)

    def gs(feat_p, ucol, vrow):
        g = torch.stack(torch.meshgrid(torch.from_numpy(vrow).double(), torch.from_numpy(ucol).double(), indexing="ij"), -1)
        return F.grid_sample(feat_p[None], torch.stack((g[..., 1], g[..., 0]), -1)[None], mode="bilinear", padding_mode="zeros",
                             align_corners=True)[0]
    for b in range(len(c.sources[0])):
        s, Kb = c.sources[0][b], c.K_in[0][b]
        D, _ = K.plane_maps64(fe, fo, c.W, s, c.voxel, Kb, c.R, c.rp)
        for p, (ac, ar) in enumerate(K.PLANE_AXES):
            patch = gs(fo[p], K.lattice32(s[ac], c.voxel, i), K.lattice32(s[ar], c.voxel, i))
            for kr in (-c.R, 0, c.R):
                for kc in (-c.R, 0, c.R):
                    shift = gs(fe[p], K.lattice32(s[ac], c.voxel, int(Kb[ac]) + kc + i), K.lattice32(s[ar], c.voxel, int(Kb[ar]) + kr + i))
                    want = float((shift - patch).abs().sum())
                    assert abs(float(D[p, kr + c.R, kc + c.R]) - want) <= 1e-12 * max(1.0, want)


def test_oracle_separable_sum_is_the_definition():
    c = K.make_case("K")
    o = K.oracle("K")[0]
    for b in range(len(c.sources[0])):
        for k in ((0, 0, 0), (-2, 1, 2), (2, 2, -2), tuple(int(v) for v in o.winner[b])):
            want = K.brute_force_D(c.edits[0], c.origs[0], c.chmap, c.W, c.sources[0][b], c.voxel, c.K_in[0][b], k, c.rp)
            idx = ((k[2] + c.R) * c.side + k[1] + c.R) * c.side + k[0] + c.R
            assert abs(float(o.D[b, idx]) - want) <= 1e-12 * want


def test_oracle_finds_a_whole_texel_roll_exactly():
    c = K.roll_case()
    o = K.track64(c.edit, c.orig, c.chmap, c.W, c.sources, c.voxel, np.zeros((1, 3), np.int32), c.R, c.rp)
    assert tuple(o.winner[0]) == c.k and float(o.D[0, o.index[0]]) == 0.0 and o.margin[0] > 1.0
    # with the roll as K_in the winner is k = 0, the same D
    o2 = K.track64(c.edit, c.orig, c.chmap, c.W, c.sources, c.voxel, np.array([c.k], np.int32), c.R, c.rp)
    assert tuple(o2.winner[0]) == (0, 0, 0) and float(o2.D[0, o2.index[0]]) == 0.0


def test_tie_rule():
    vol = torch.ones(3, 3, 3, dtype=torch.float64)
    assert K.winner_of(vol, 1)[0] == (0, 0, 0)                        # all equal: the smallest |k|^2
    vol[1, 1, 1] = 2.0
    assert K.winner_of(vol, 1)[0] == (0, 0, -1) and K.winner_of(vol, 1)[2] == 0.0     # |k|^2 = 1 six times: the lowest index, kz = -1
    vol[0, 1, 1] = 2.0
    assert K.winner_of(vol, 1)[0] == (0, -1, 0)
    vol[2, 2, 2] = 0.5
    assert K.winner_of(vol, 1)[0] == (1, 1, 1) and K.winner_of(vol, 1)[2] == 0.5


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("name", K.CASES)
def test_case_input_conditions(name):
    """Outside the explicit tie handles the oracle's runner-up exceeds its winner by four times the comparison tolerance (the
    largest over the handle's candidates); a tie handle shares an exact D = 0 between k = 0 and other candidates.  Every handle is
    one or the other."""
    c, o = K.make_case(name), K.oracle(name)
    ties = K.TIE_HANDLES.get(name, set())
    for e in range(c.E):
        assert o[e].D.shape == (len(c.sources[e]), c.side ** 3) and bool(torch.isfinite(o[e].D).all())
        for b in range(len(c.sources[e])):
            if (e, b) in ties:
                # no sample of the patch or of the winner's window is inside the map: an exact 0 in any precision, shared with other
                # candidates; every candidate that does read features is clear of it
                D = o[e].D[b]
                assert o[e].margin[b] == 0.0 and float(D[o[e].index[b]]) == 0.0 and tuple(o[e].winner[b]) == (0, 0, 0)
                assert float(D[D > 0].min()) >= 4 * float(K.tolerance(o[e].M[b], c.R, c.rp, c.Cc).max())
            elif c.R > 0:
                tol = float(K.tolerance(o[e].M[b], c.R, c.rp, c.Cc).max())
                assert o[e].margin[b] >= 4 * tol, (name, e, b, o[e].margin[b], tol)


def test_cases_cover_what_they_are_for():
    assert {K.make_case(n).Cc for n in K.CASES} >= {20, 70, 64, 8, 170}
    assert {K.make_case(n).R for n in K.CASES} >= {0, 1, 2, 3} and {K.make_case(n).rp for n in K.CASES} >= {0, 1, 2}
    assert {K.chunk_width(K.make_case(n).R, K.make_case(n).rp) for n in K.CASES} == {64, 32, 16}
    assert any(K.make_case(n).Cc % K.chunk_width(K.make_case(n).R, K.make_case(n).rp) for n in K.CASES)      # a part-filled chunk
    # the rolled cases move the winner off k = 0
    assert any(tuple(w) != (0, 0, 0) for n in ("A", "G") for w in K.oracle(n)[0].winner)
    # K: K_in + k takes both signs and 0 on some axis
    k = K.make_case("K")
    tot = k.K_in[0][:, None, :] + np.arange(-k.R, k.R + 1)[None, :, None]
    assert (tot < 0).any() and (tot > 0).any() and (tot == 0).any()
    # F: the window (patch included) leaves the map on every side, as a column and as a row
    f = K.make_case("F")
    m = np.arange(-(f.R + f.rp), f.R + f.rp + 1)
    tex = (K.lattice32(f.sources[0][:, :, None], f.voxel, m[None, None, :]).astype(np.float64) + 1) * (f.W - 1) / 2
    for axes in ((0, 1), (1, 2)):          # column axes of the planes, row axes of the planes
        t = tex[:, list(axes)]
        assert (t < -1).any() and (t > f.W).any() and ((t > 0) & (t < f.W - 1)).any()
    L, Ls = K.make_case("L"), K.make_case("Ls")
    assert L.offsets == [0, 1, 4, 6] and L.origs.shape[0] == 3 and Ls.origs.shape[0] == 1 and torch.equal(L.edits, Ls.edits)


# ------------------------------------------------------------------------------------------------ ABI 21
def test_abi_declares_and_binds_the_tracking_calls():
    from ishapediting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ishap.h")).read()
    declared = set(re.findall(r"\b(ishap_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("ishap_drag_track", "ishap_drag_track_scratch_bytes"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name)
    assert L.ishap_version() >= 21


def test_scratch_bytes_formula_and_its_refusals():
    from ishapediting_amd import _lib
    f = _lib.lib().ishap_drag_track_scratch_bytes
    for E, B, Rs, rp, Cc in ((1, 1, 0, 0, 1), (1, 2, 2, 1, 20), (3, 6, 3, 2, 70), (1, 1, 4, 2, 170), (1, 16, 8, 4, 170), (32, 32, 8, 0, 64),
                             (2, 5, 4, 4, 33)):
        assert f(E, B, Rs, rp, Cc) == K.scratch_bytes(E, B, Rs, rp, Cc) > 0
    for bad in ((0, 1, 2, 1, 20), (33, 40, 2, 1, 20), (2, 1, 2, 1, 20), (1, 1, -1, 1, 20), (1, 1, 9, 1, 20), (1, 1, 2, -1, 20),
                (1, 1, 2, 5, 20), (1, 1, 2, 1, 0), (1, 0, 2, 1, 20)):
        assert f(*bad) == -1 == K.scratch_bytes(*bad)
    assert K.chunk_width(4, 2) == 64 and K.chunk_width(8, 0) == 32 and K.chunk_width(8, 4) == 16
    assert K.chain_length(4, 2, 170) == 25 + 6 + 3 + 2


KERNELS = ("track_corr_kernelILi64E", "track_corr_kernelILi32E", "track_corr_kernelILi16E", "track_argmin_kernel")


def test_tracking_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for name in KERNELS:
        mine = [n for n in ks if name in n]
        assert len(mine) == 1, (name, mine)
        k = ks[mine[0]]
        assert k.get(".private_segment_fixed_size", 0) == 0, (mine[0], k.get(".private_segment_fixed_size"))
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (mine[0], k)
