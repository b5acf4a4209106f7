"""Quadric vertex clustering without a GPU: the ABI (version 26, symbols, prototypes, every refusal called with a fake address so
that a call which got as far as a launch or a memset would not return), the scratch-size formula, the code-object metadata of
the new kernels (tools/kernel_meta.py: no private segment, no spills), the numpy reference (tests/simplify_ref.py) against a
brute-force restatement with Python integers on tiny hand meshes, and the reference's invariants on the fixture meshed with the
CPU marching cubes of oracle/surface_cpu.py."""
import ctypes as C
import math
import os
import sys
from functools import lru_cache

import numpy as np
import pytest

from tests import simplify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
NEW = {
    "ishap_mesh_simplify_scratch_bytes": (C.c_longlong, 3),
    "ishap_mesh_simplify_count": (C.c_int, 12),
    "ishap_mesh_simplify_emit": (C.c_int, 16),
}
KERNELS = ("simplify_mark_kernel", "simplify_popc_kernel", "simplify_sum_counters_kernel", "simplify_clear_rows_kernel", "simplify_vertex_sums_kernel",
           "simplify_quadric_sums_kernel", "simplify_insert_kernel", "simplify_survivors_kernel", "simplify_mark_ref_kernel",
           "simplify_guard_kernel", "simplify_emit_vertices_kernel", "simplify_emit_triangles_kernel", "simplify_emit_map_kernel")
CELLS = (0.75, 2, 3.3, 4, 8)


def lib():
    from ishapediting_amd import _lib
    return _lib


def err():
    m = lib().lib().ishap_last_error()
    return m.decode() if m else ""


def i3(a, b, c):
    return (C.c_int * 3)(a, b, c)


def d3(a, b, c):
    return (C.c_double * 3)(a, b, c)


def test_abi_and_prototypes():
    L = lib().lib()
    assert L.ishap_version() >= 26
    header = open(os.path.join(ROOT, "include", "ishap.h")).read()
    for name, (res, nargs) in NEW.items():
        assert name in lib().SYMBOLS, name
        got_res, got_args = lib().SYMBOLS[name]
        assert got_res is res and len(got_args) == nargs, (name, got_res, len(got_args))
        assert getattr(L, name).restype is res
        assert f"{name}(" in header, f"{name} is not declared in include/ishap.h"
    assert "Mesh simplification" in header and "rint(value 2^36)" in header       # the rule is stated there


def test_refusals_launch_nothing():
    L = lib().lib()
    lo, dims, big = d3(0, 0, 0), i3(4, 4, 4), 1 << 40

    def count(verts=FAKE, nv=10, tris=FAKE, nt=10, lo=lo, h=1.0, dims=dims, mode=0, scratch=FAKE, nbytes=big, counts=FAKE):
        return L.ishap_mesh_simplify_count(verts, nv, tris, nt, lo, h, dims, mode, scratch, nbytes, counts, None)

    def emit(verts=FAKE, nv=10, tris=FAKE, nt=10, lo=lo, h=1.0, dims=dims, mode=0, reg=1e-3, scratch=FAKE, nbytes=big, ov=FAKE, ot=FAKE,
             vm=FAKE, vc=None):
        return L.ishap_mesh_simplify_emit(verts, nv, tris, nt, lo, h, dims, mode, reg, scratch, nbytes, ov, ot, vm, vc, None)

    for call in (count, emit):
        for kw in ({"verts": None}, {"tris": None}, {"lo": None}, {"dims": None}, {"scratch": None}):
            assert call(**kw) == -2 and "null" in err().lower(), (call.__name__, kw, err())
        for h in (0.0, -1.0, float("inf"), float("nan")):
            assert call(h=h) == -2 and "cell size" in err(), (h, err())
        assert call(lo=d3(0, float("nan"), 0)) == -2 and "origin" in err()
        for bad in (i3(0, 4, 4), i3(4, -1, 4), i3(4, 4, 0)):
            assert call(dims=bad) == -2 and "dim" in err(), err()
        for bad in (i3(1025, 1024, 1024), i3(1 << 16, 1 << 16, 1), i3(0x7fffffff, 0x7fffffff, 0x7fffffff)):
            assert call(dims=bad) == -2 and "2^30" in err(), err()
        assert call(dims=i3(1024, 1024, 1024), nbytes=1 << 20) == -2 and "scratch" in err()      # 2^30 cells themselves are allowed
        assert call(nbytes=64) == -2 and "scratch" in err()
        assert call(scratch=FAKE + 4) == -2 and "aligned" in err()
        for mode in (-1, 2):
            assert call(mode=mode) == -2 and "contraction" in err()
        assert call(nt=(1 << 31) // 3 + 1) == -2 and "ntris" in err()
        assert call(nv=1 << 31) == -2 and "nverts" in err()
        assert call(nv=-1) == -2 and call(nt=-1) == -2
        assert call(nt=1 << 62) == -2 and "ntris" in err()       # 3 * ntris is never formed
    assert count(counts=None) == -2 and "null" in err().lower()
    assert emit(ov=None) == -2 and "null" in err().lower()
    assert emit(ot=None) == -2 and "null" in err().lower()
    assert emit(vm=None) == -2 and "null" in err().lower()
    for reg in (0.0, -1e-3, float("inf"), float("nan")):
        assert emit(reg=reg) == -2 and "regularization" in err()


def layout_bytes(nv, nt, dims):
    """the scratch layout of csrc/simplify.h"""
    up = lambda a: (a + 255) // 256 * 256
    cells = dims[0] * dims[1] * dims[2]
    words, cmax, table = (cells + 31) // 32, min(nv, cells), 64
    while table < 2 * nt:
        table *= 2
    at = 512
    for part in (4 * words, 4 * words, 4 * nv, 128 * cmax, 4 * (cmax + 1), 4 * table, 4 * (nt + 1)):
        at = up(at + part)
    longest = max(words, cmax + 1, nt + 1)
    return up(at + 4 * ((longest + 2047) // 2048 + 1))


def test_scratch_bytes():
    L = lib().lib()
    for nv, nt, dims in ((0, 0, (1, 1, 1)), (3, 1, (1, 1, 1)), (2716, 5424, (17, 17, 17)), (65, 257, (65, 64, 64)), (12, 4, (1024, 1024, 1024)),
                         (10_000_000, 20_000_000, (512, 512, 512))):
        assert L.ishap_mesh_simplify_scratch_bytes(nv, nt, i3(*dims)) == layout_bytes(nv, nt, dims), (nv, nt, dims)
    assert L.ishap_mesh_simplify_scratch_bytes(12, 4, i3(1024, 1024, 1024)) >= 2 * (1 << 27)       # bitmap and ranks at the cell limit
    for nv, nt, dims in ((-1, 1, (1, 1, 1)), (1, -1, (1, 1, 1)), (1 << 31, 1, (1, 1, 1)), (1, (1 << 31) // 3 + 1, (1, 1, 1)), (1, 1 << 62, (1, 1, 1)), (1, 1, (0, 1, 1)),
                         (1, 1, (1025, 1024, 1024))):
        assert L.ishap_mesh_simplify_scratch_bytes(nv, nt, i3(*dims)) == -1, (nv, nt, dims)
    assert L.ishap_mesh_simplify_scratch_bytes(1, 1, None) == -1


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for name in KERNELS:
        mine = [n for n in ks if name in n]
        assert len(mine) == 1, (name, mine)
        k = ks[mine[0]]
        assert k.get(".private_segment_fixed_size", 0) == 0, (mine[0], k.get(".private_segment_fixed_size"))
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (mine[0], k)
        # streaming kernels: full occupancy; the quadric pass holds a triangle's float64 arithmetic and is bounded by its LDS
        # (42 KB a workgroup: three per compute unit, twelve waves), which 128 registers do not lower
        assert k.get(".vgpr_count", 0) <= (128 if name == "simplify_quadric_sums_kernel" else 64), (mine[0], k.get(".vgpr_count"))
        assert k.get(".group_segment_fixed_size", 0) <= 43008, (mine[0], k.get(".group_segment_fixed_size"))


def test_command_line_options():
    from ishapediting_amd import generate
    assert generate.build_parser().parse_args(["--mesh_simplify", "2.5"]).mesh_simplify == 2.5
    assert generate.build_parser().parse_args([]).mesh_simplify is None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import headless_edit
    assert headless_edit.build_parser().parse_args(["--simplify", "2"]).simplify == 2.0
    assert headless_edit.build_parser().parse_args([]).simplify is None


def test_simplify_keyword_is_checked():
    from ishapediting_amd import mesh
    assert mesh._checked_simplify(None) is None
    assert mesh._checked_simplify(2) == {"cell": 2.0}
    assert mesh._checked_simplify({"cell": 3, "contraction": "average"}) == {"cell": 3.0, "contraction": "average"}
    for bad in ({"contraction": "quadric"}, {"cell": 2, "size": 1}, {"cell": 0}, {"cell": float("nan")}, -1.0,
                {"cell": 2, "contraction": "median"}):
        with pytest.raises(ValueError):
            mesh._checked_simplify(bad)


# ------------------------------------------------------------------------------------------------ the reference against brute force
def brute(verts, tris, lo, h, dims, contraction, lam=1e-3):
    """the rule once more, one vertex and one triangle at a time, Python floats and integers"""
    verts = np.asarray(verts, np.float32)
    V = len(verts)
    f = lambda x: float(x)
    loc = []
    for v in verts:
        c, q, p = [], [], []
        for a in range(3):
            qa = (f(v[a]) - f(lo[a])) / f(h)
            t = math.floor(qa) if math.isfinite(qa) else (0 if math.isnan(qa) else (-1 if qa < 0 else dims[a]))
            ca = min(max(t, 0), dims[a] - 1)
            pa = qa - (ca + 0.5)
            pa = 0.0 if math.isnan(pa) else min(max(pa, -0.5), 0.5)
            c.append(ca); q.append(qa); p.append(pa)
        loc.append(((c[0] * dims[1] + c[1]) * dims[2] + c[2], c, q, p))
    ids = sorted({l[0] for l in loc})
    cl = [ids.index(l[0]) for l in loc]
    sums = [[0] * 16 for _ in ids]
    for s in sums:
        s[4] = V
    for i, (_, c, q, p) in enumerate(loc):
        s = sums[cl[i]]
        s[0] += 1
        for a in range(3):
            s[1 + a] += int(np.rint(p[a] * 2.0 ** 32))
        s[4] = min(s[4], i)
    kept, seen, nondeg = [], set(), 0
    for tri in np.asarray(tris).tolist():
        if any(i < 0 or i >= V for i in tri):
            continue
        if contraction == "quadric":
            P = [loc[i][2] for i in tri]
            u = [P[1][a] - P[0][a] for a in range(3)]
            w_ = [P[2][a] - P[0][a] for a in range(3)]
            N = [u[1] * w_[2] - u[2] * w_[1], u[2] * w_[0] - u[0] * w_[2], u[0] * w_[1] - u[1] * w_[0]]
            L = math.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
            if L > 0 and math.isfinite(L):
                n, w = [x / L for x in N], 0.5 * L
                for i in tri:
                    p, s = loc[i][3], sums[cl[i]]
                    d = -((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2])
                    e = [n[0], n[1], n[2], d]
                    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3))):
                        s[5 + j] += int(np.rint((w * (e[a] * e[b])) * 2.0 ** 36))
                    s[15] += math.ceil(w)
        k = [cl[i] for i in tri]
        if len(set(k)) < 3:
            continue
        nondeg += 1
        m = k.index(min(k))
        key = (k[m], k[(m + 1) % 3], k[(m + 2) % 3])
        if key not in seen:
            seen.add(key)
            kept.append(key)
    ref = sorted({c for key in kept for c in key})
    rank = {c: r for r, c in enumerate(ref)}
    out = []
    for c in ref:
        s = sums[c]
        if s[0] == 1:
            out.append(verts[s[4]])
            continue
        mean = [float(s[1 + a]) / (float(s[0]) * 2.0 ** 32) for a in range(3)]
        x = mean
        A = np.array([[s[5], s[6], s[7]], [s[6], s[8], s[9]], [s[7], s[9], s[10]]], np.float64) / 2.0 ** 36
        tr = (A[0, 0] + A[1, 1]) + A[2, 2]
        if contraction == "quadric" and tr != 0:
            M, r = A + lam * tr * np.eye(3), lam * tr * np.array(mean) - np.array(s[11:14], np.float64) / 2.0 ** 36
            det = np.linalg.det(M)
            x = [np.linalg.det(np.column_stack([r if b == a else M[:, b] for b in range(3)])) / det for a in range(3)]     # Cramer
        cc = loc[s[4]][1]
        out.append(np.array([f(lo[a]) + f(h) * ((cc[a] + 0.5) + min(max(x[a], -0.5), 0.5)) for a in range(3)]).astype(np.float32))
    vmap = [rank.get(c, -1) for c in cl]
    return (np.array(out, np.float32).reshape(-1, 3), np.array([[rank[c] for c in key] for key in kept], np.int32).reshape(-1, 3),
            np.array(vmap, np.int32), np.array(sums, dtype=object), nondeg)


def hand_meshes():
    rng = np.random.default_rng(7)
    # a random soup in a 3 x 2 x 4 grid: duplicates, reversed duplicates, degenerate and zero-area triangles, an invalid index,
    # vertices outside the grid on both sides
    v = rng.uniform(-0.4, 3.4, size=(40, 3)).astype(np.float32) * np.array([1.0, 0.66, 1.33], np.float32)
    t = rng.integers(0, 40, size=(120, 3))
    t[5] = t[4][[1, 2, 0]]
    t[6] = t[4][[0, 2, 1]]
    t[7] = (1, 1, 2)
    t[8] = (3, 40, 2)
    yield "soup", v, t, (0.0, 0.0, 0.0), 1.0, (3, 2, 4)
    yield "soup, odd origin and cell", v, t, (-0.37, 0.11, 0.2), 0.83, (5, 3, 6)
    # a flat fan in the plane z = 0.25 over 2 x 2 x 1 cells: A has rank 1, the regularisation decides the other two directions
    ang = np.linspace(0, 2 * np.pi, 13)[:-1]
    fv = np.concatenate([[[1.0, 1.0, 0.25]], np.stack([1 + 0.9 * np.cos(ang), 1 + 0.9 * np.sin(ang), np.full(12, 0.25)], 1)]).astype(np.float32)
    ft = np.array([[0, 1 + k, 1 + (k + 1) % 12] for k in range(12)])
    yield "flat fan", fv, ft, (0.0, 0.0, 0.0), 1.0, (2, 2, 1)
    # non-finite vertices: cell 0 or the border, their triangles add no quadric
    nv = v.copy()
    nv[0, 0], nv[1, 1], nv[2, 2] = np.nan, np.inf, -np.inf
    yield "non-finite", nv, t, (0.0, 0.0, 0.0), 1.0, (3, 2, 4)


@pytest.mark.parametrize("contraction", ["quadric", "average"])
def test_reference_against_brute_force(contraction):
    for name, v, t, lo, h, dims in hand_meshes():
        got = R.simplify(v, t, lo, h, dims, contraction)
        bv, bt, bmap, bsums, bnondeg = brute(v, t, lo, h, dims, contraction)
        assert got.nondegenerate == bnondeg and got.tris.shape[0] > 0, name
        assert np.array_equal(got.tris, bt) and np.array_equal(got.vertex_map, bmap), name
        used = (0, 1, 2, 3, 4) if contraction == "average" else range(16)
        for j in used:
            assert [int(x) for x in got.sums[:, j]] == [int(x) for x in bsums[:, j]], (name, j)
        assert got.verts.shape == bv.shape
        single = got.counts[got.referenced] == 1
        assert np.array_equal(got.verts[single].view(np.uint32), bv[single].view(np.uint32)), name
        # two direct methods on a matrix of condition <= 1001: far inside one float32 ulp of coordinates below 8
        assert np.allclose(got.verts, bv, rtol=0, atol=1e-6, equal_nan=True), (name, np.abs(got.verts - bv).max())
    with pytest.raises(R.Overflow):
        big = np.array([[0.1, 0.1, 0.1], [2.0 ** 14, 0.1, 0.1], [0.1, 2.0 ** 14, 0.1], [0.2, 0.3, 2.5]], np.float32)
        R.simplify(big, [[0, 1, 2], [0, 1, 3], [0, 3, 2], [3, 1, 2]], (0, 0, 0), 1.0, (2, 2, 3))     # w = 2^27 in cell 0


# ------------------------------------------------------------------------------------------------ invariants on the fixture
@lru_cache(maxsize=None)
def cpu_fixture(res):
    import torch
    from oracle.surface_cpu import marching_cubes
    out = marching_cubes(torch.from_numpy(R.fixture_volume(res)), 0.0)
    return np.asarray(out[0], np.float32), np.asarray(out[1], np.int64)


@pytest.mark.parametrize("res", [33, 41])
@pytest.mark.parametrize("contraction", ["quadric", "average"])
def test_reference_invariants(res, contraction):
    v, t = cpu_fixture(res)
    assert v.shape[0] > 2000 and t.shape[0] > 5000
    seen_unreferenced = False
    for cell in CELLS:
        g = int(np.floor((res - 1) / cell)) + 1
        r = R.simplify(v, t, (0.0, 0.0, 0.0), cell, (g, g, g), contraction)
        C_, Vo = len(r.cells), r.verts.shape[0]
        assert 0 < Vo <= C_ < v.shape[0] and 0 < r.tris.shape[0] <= r.nondegenerate < t.shape[0]
        assert Vo == int(r.referenced.sum()) and r.counts.sum() == v.shape[0]
        seen_unreferenced |= Vo < C_
        # representatives stay inside their cells (closed, up to the float32 rounding of the output coordinate)
        cc = np.stack([r.cells // (g * g), (r.cells // g) % g, r.cells % g], 1)[r.referenced].astype(np.float64)
        ulp = np.spacing(np.abs(r.verts).astype(np.float32)).astype(np.float64)
        assert (r.verts >= cc * cell - ulp).all() and (r.verts <= (cc + 1) * cell + ulp).all()
        # each mapped input vertex is within h per axis of its representative
        m = r.vertex_map >= 0
        assert (np.abs(v[m].astype(np.float64) - r.verts[r.vertex_map[m]]) <= cell + ulp[r.vertex_map[m]]).all()
        assert np.array_equal(r.vertex_map[m], (np.cumsum(r.referenced) - 1)[r.cluster[m]]) and (~r.referenced[r.cluster[~m]]).all()
        # the triangle rules: three distinct corners, smallest first, no rotated triple twice, every output vertex used, the
        # order of the input kept
        tr = r.tris
        assert (tr[:, 0] < tr[:, 1]).all() and (tr[:, 0] < tr[:, 2]).all() and (tr[:, 1] != tr[:, 2]).all()
        assert len(np.unique(tr, axis=0)) == len(tr) and np.array_equal(np.unique(tr), np.arange(Vo))
        rank = np.cumsum(r.referenced) - 1
        ct = r.cluster[t]
        ok = (ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2])
        rot = rank[R.rotate(ct[ok])]
        first = {}
        for k, key in enumerate(map(tuple, rot.tolist())):
            first.setdefault(key, k)
        assert [tuple(x) for x in tr.tolist()] == sorted(first, key=first.get)
        if contraction == "quadric":
            assert (r.bound <= 3e-5).all() and (r.sums[r.referenced, 15] < R.GUARD).all()
    if res == 33:
        assert seen_unreferenced, "no fixture / cell pair has an unreferenced cluster"
