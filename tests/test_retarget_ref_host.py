"""The float64 statement of the closed-loop re-aim (tests/retarget_ref.py) pinned on the host: its own invariants, the input
conditions of every case of the device tests, the ABI, and the `closed_loop` keyword's parsing.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import retarget_ref as Q

INF = float("inf")


# ------------------------------------------------------------------------------------------------ the oracle's invariants
@pytest.mark.parametrize("name", Q.CASES)
def test_step_inf_gives_the_targets_bit_for_bit(name):
    c = Q.make_case(name)
    for e in range(c.E):
        o = Q.reaim64(c.sources[e], c.targets[e], c.K[e], c.voxel, INF, c.arrive)
        assert o.hold.all()
        assert np.array_equal(o.goals.view(np.uint32), np.asarray(c.targets[e], np.float32).view(np.uint32))


@pytest.mark.parametrize("name", Q.CASES)
def test_the_goal_lies_on_the_segment_at_distance_step(name):
    c = Q.make_case(name)
    vx = np.float64(np.float32(c.voxel))
    for e in range(c.E):
        for step in (0.5, 1.0, c.step if np.isfinite(c.step) else 2.0):
            o = Q.reaim64(c.sources[e], c.targets[e], c.K[e], c.voxel, step, c.arrive)
            s, t = c.sources[e].astype(np.float64), c.targets[e].astype(np.float64)
            pos = c.K[e].astype(np.float64)                       # the handle, in voxels from the source
            T = (t - s) / vx
            for b in np.nonzero(~o.hold)[0]:
                g = (o.goals64[b] - s[b]) / vx                    # the goal before its rounding to float, same units
                assert abs(np.linalg.norm(g - pos[b]) - step) <= 1e-12 * max(1.0, step), (name, e, b)
                lam = np.dot(g - pos[b], T[b] - pos[b]) / np.dot(T[b] - pos[b], T[b] - pos[b])
                assert 0.0 < lam < 1.0                            # between the handle and the target ...
                off = (g - pos[b]) - lam * (T[b] - pos[b])
                assert np.linalg.norm(off) <= 1e-12 * max(1.0, o.d[b])      # ... and on the line through them
            for b in np.nonzero(o.hold)[0]:
                assert o.d[b] <= step and np.array_equal(o.goals[b], np.asarray(c.targets[e], np.float32)[b])


@pytest.mark.parametrize("name", Q.CASES)
def test_arrival_is_monotone_in_arrive(name):
    c = Q.make_case(name)
    for e in range(c.E):
        last = None
        for arrive in (0.0, 0.25, 1.0, 2.5, 8.0, 40.0, INF):
            o = Q.reaim64(c.sources[e], c.targets[e], c.K[e], c.voxel, c.step, arrive)
            if last is not None:
                assert (o.arrived >= last).all()
            assert o.done == bool(o.arrived.all())
            last = o.arrived
        assert last.all()                                         # arrive = inf: everything has arrived


# ------------------------------------------------------------------------------------------------ the cases' input conditions
@pytest.mark.parametrize("name", Q.CASES)
def test_no_distance_sits_on_a_threshold(name):
    c = Q.make_case(name)
    for e, o in enumerate(Q.oracle(name)):
        for b, d in enumerate(o.d):
            if d == 0.0:
                continue
            assert abs(d - c.step) > Q.MARGIN and abs(d - c.arrive) > Q.MARGIN, (name, e, b, d)
        assert 3 * c.W * c.W <= Q.LDS_BYTES and (3 * c.W * c.W) % 4 == 0 and c.ld % 8 == 0


def test_the_cases_cover_what_they_are_there_for():
    a = Q.make_case("A")
    assert a.E == 1 and len(a.sources[0]) == 2 and not a.K[0].any()
    k, ko = Q.make_case("K"), Q.oracle("K")[0]
    assert (k.K[0] > 0).any() and (k.K[0] < 0).any()
    assert ko.hold[0] and ko.d[0] > 0 and not ko.hold[1] and ko.d[2] == 0.0 and ko.hold[2]
    T = (k.targets[0].astype(np.float64) - k.sources[0].astype(np.float64)) / np.float64(np.float32(k.voxel))
    assert (np.sign(T[0] - k.K[0]) != np.sign(T[0])).any()                  # handle 0 has crossed its target on some axis
    assert np.array_equal(T[2], k.K[0][2].astype(np.float64))               # handle 2: K = T exactly
    f, fo = Q.make_case("F"), Q.oracle("F")[0]
    W = f.W
    assert fo.hold[0] and fo.hold[3] and not fo.hold[1]
    for coord in (1.0, -1.05):                                              # as a column and as a row of some plane
        col = {p for p, (ac, ar) in enumerate(Q.PLANE_AXES) for b in (0, 3) if fo.goals[b, ac] == np.float32(coord)}
        row = {p for p, (ac, ar) in enumerate(Q.PLANE_AXES) for b in (0, 3) if fo.goals[b, ar] == np.float32(coord)}
        assert col and row, coord
        lat = Q._round_texel(Q.lattice32(np.array([coord], np.float32), f.voxel, f.r)[0], W)
        assert ((lat < 0) | (lat >= W)).any() and ((lat >= 0) & (lat < W)).any()       # marks inside and outside the map
    l, lo = Q.make_case("L"), Q.oracle("L")
    assert [len(s) for s in l.sources] == [1, 3, 2] and lo[0].done and not (lo[1].done and lo[2].done)
    j = Q.make_case("J")
    assert (j.W, j.ld, j.r, len(j.sources[0])) == (64, 512, 12, 3) and j.voxel == 2 / 256
    assert Q.make_case("INF").step == INF and all(o.hold.all() for o in Q.oracle("INF"))
    # both branches and both answers occur somewhere in the table
    holds = np.concatenate([o.hold for n in Q.CASES for o in Q.oracle(n)])
    arr = np.concatenate([o.arrived for n in Q.CASES for o in Q.oracle(n)])
    assert holds.any() and (~holds).any() and arr.any() and (~arr).any()


@pytest.mark.parametrize("name", ("A", "K", "F", "L"))
def test_bit_0_of_the_host_builder_is_the_references_mask_sets(name):
    c = Q.make_case(name)
    for e, o in enumerate(Q.oracle(name)):
        setup = O.DragSetup(c.sources[e], o.goals, c.r, c.voxel, c.W)
        for p in range(3):
            assert np.array_equal((o.touched[p] & 1) == 0, setup.masks[p].numpy()), (name, e, p)
        assert o.nmask == sum(int(m.sum()) for m in setup.masks) and o.nmask > 0
        assert ((o.touched & 2) != 0).any()
        # bit 1 covers every bilinear corner of a goal position that lies in the map
        g = setup.shift_grid.double()
        ix, iy = (g[..., 0] + 1) / 2 * (c.W - 1), (g[..., 1] + 1) / 2 * (c.W - 1)
        for p in range(3):
            for dx in (0, 1):
                for dy in (0, 1):
                    x, y = torch.floor(ix[p]).long() + dx, torch.floor(iy[p]).long() + dy
                    ok = (x >= 0) & (x < c.W) & (y >= 0) & (y < c.W)
                    assert bool((torch.from_numpy(o.touched[p])[y[ok], x[ok]] & 2).bool().all())


def test_ulps32():
    one = np.float32(1.0)
    assert Q.ulps32(np.array([one]), np.array([np.nextafter(one, np.float32(2))]))[0] == 1
    assert Q.ulps32(np.array([0.0], np.float32), np.array([-0.0], np.float32))[0] == 0
    tiny = np.float32(1e-45)
    assert Q.ulps32(np.array([tiny]), np.array([-tiny]))[0] == 2


# ------------------------------------------------------------------------------------------------ the ABI
def test_abi_22_exports_the_retarget_calls():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert int(L.ishap_version()) >= 22
    assert hasattr(L, "ishap_drag_batch_retarget") and hasattr(L, "ishap_drag_batch_retarget_each")


# ------------------------------------------------------------------------------------------------ the keyword
def test_closed_loop_options():
    from ishapediting_amd.drag_utils import CLOSED_LOOP_DEFAULTS, closed_loop_options, closed_loop_track
    assert closed_loop_options(None) is None and closed_loop_options(False) is None
    assert closed_loop_options(True) == CLOSED_LOOP_DEFAULTS == {"step": 2.0, "arrive": 1.0, "stop": False, "lag": 2}
    assert closed_loop_options({"step": INF, "stop": True}) == {"step": INF, "arrive": 1.0, "stop": True, "lag": 2}
    assert closed_loop_options({"arrive": 0, "lag": 3})["arrive"] == 0.0
    for bad, word in (({"step": 0}, "step"), ({"step": -1.0}, "step"), ({"step": float("nan")}, "step"), ({"step": "far"}, "step"),
                      ({"arrive": -0.5}, "arrive"), ({"arrive": float("nan")}, "arrive"), ({"lag": 0}, "lag"), ({"lag": 1.5}, "lag"),
                      ({"stop": "yes"}, "stop"), ({"steps": 2.0}, "unknown"), (3, "dict")):
        with pytest.raises(ValueError, match=word):
            closed_loop_options(bad)
    # a batch: one dict, or one per edit for step and arrive
    assert closed_loop_options({"step": 1.0}, 3)["step"] == 1.0
    per = closed_loop_options([{"step": 1.0}, True, {"arrive": 0.5}], 3)
    assert per["step"] == [1.0, 2.0, 2.0] and per["arrive"] == [1.0, 1.0, 0.5] and per["stop"] is False and per["lag"] == 2
    with pytest.raises(ValueError, match="entries"):
        closed_loop_options([True, True], 3)
    with pytest.raises(ValueError, match="stop and lag"):
        closed_loop_options([{"stop": True}, True], 2)
    with pytest.raises(ValueError, match=r"closed_loop\[1\]"):
        closed_loop_options([True, {"step": 0}], 2)
    # it implies tracking
    assert closed_loop_track(None, None) is None and closed_loop_track(None, {"radius": 2}) == {"radius": 2}
    opts = closed_loop_options(True)
    assert closed_loop_track(opts, None) is True and closed_loop_track(opts, {"every": 2}) == {"every": 2}
    with pytest.raises(ValueError, match="track"):
        closed_loop_track(opts, False)
