"""Which kernel every implicit-GEMM launch gets: the K split and kernel form that csrc/igemm.hip plans (igemm_plan_ksplit,
igemm_plan), read on the CPU through ishap_igemm_plan.  The expected values are what the dispatch chose before it was gathered
into the planner (the executor's split overrides, igemm_launch's tile pick, the igemm2 / igemm4 ladders and the profiling slot
conditional), evaluated for these shapes -- not values read back from the planner."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: ((M = images*H*W, Cin, Cout, taps, K2, H, W, pending, epilogue sums), (K split, profiling slot, kernel))
CASES = {
    "skinny 1x1 on an 8x8 map": ((64, 1024, 1024, 1, 0, 8, 8, 0, 0), (1, 5, "igemm_skinny_kernel<2, false>")),
    "skinny 1x1, pending but K < 2048": ((64, 1024, 1024, 1, 0, 8, 8, 1, 0), (1, 5, "igemm_skinny_kernel<2, false>")),
    "sliced 1x1, K = 3072": ((64, 3072, 1024, 1, 0, 8, 8, 1, 0), (16, 3, "igemm2_kernel<64, 64, 4, false, 1>")),
    "sliced 1x1, K = 2048": ((64, 2048, 1024, 1, 0, 8, 8, 1, 0), (8, 3, "igemm2_kernel<64, 64, 4, false, 1>")),
    "3x3 on an 8x8 map, small-map slices": ((64, 1024, 1024, 9, 0, 8, 8, 1, 0), (16, 11, "igemm4_kernel<64, 64, 8, 4, 3, 1>")),
    "3x3 on an 8x8 map, folded source": ((64, 1024, 1024, 9, 2048, 8, 8, 1, 0), (16, 11, "igemm4_kernel<64, 64, 8, 4, 3, 1>")),
    "3x3 on an 8x8 map, generic split": ((64, 1024, 1024, 9, 0, 8, 8, 0, 1), (16, 11, "igemm4_kernel<64, 64, 8, 4, 3, 1>")),
    "3x3 128-tile": ((16384, 256, 256, 9, 0, 128, 128, 0, 1), (1, 8, "igemm4_kernel<128, 128, 128, 5, 3, 1>")),
    "3x3 128-tile, folded source": ((16384, 256, 256, 9, 512, 128, 128, 0, 0), (1, 8, "igemm4_kernel<128, 128, 128, 5, 3, 1>")),
    "3x3 64-tile, folded source: igemm2": ((4096, 256, 512, 9, 512, 64, 64, 0, 0), (1, 1, "igemm2_kernel<64, 64, 4, true, 1>")),
    "3x3 64-tile, folded source: igemm2 two-team": ((1024, 512, 512, 9, 1280, 32, 32, 0, 0), (2, 4, "igemm2_kernel<64, 64, 4, true, 2>")),
    "1x1 128-tile": ((32768, 128, 128, 1, 0, 64, 64, 0, 0), (1, 2, "igemm2_kernel<128, 128, 4, false, 1>")),
    "1x1, sums need H*W % 128 for the 128-tile": ((32768, 128, 128, 1, 0, 4, 16, 0, 1), (1, 3, "igemm2_kernel<64, 64, 4, false, 1>")),
    "3x3 128-tile on 8x8 maps: igemm2": ((32768, 128, 128, 9, 0, 8, 8, 0, 0), (1, 0, "igemm2_kernel<128, 128, 4, true, 1>")),
    "3x3 with Cin % 64 != 0: BK = 32": ((32768, 96, 128, 9, 0, 128, 128, 0, 0), (1, 6, "igemm_kernel<64, 64, 32, 2, 2, true>")),
    "1x1 with K % 64 != 0: BK = 32": ((4096, 96, 256, 1, 0, 64, 64, 0, 0), (1, 6, "igemm_kernel<64, 64, 32, 2, 2, false>")),
    "halo tiles 64^2": ((4096, 256, 256, 9, 0, 64, 64, 0, 1), (1, 7, "igemm4_halo_kernel<64, 6>")),
    "halo tiles 32^2, 2 slices": ((1024, 512, 512, 9, 0, 32, 32, 0, 1), (2, 7, "igemm4_halo_kernel<32, 6>")),
    "halo tiles 16^2, 4 slices": ((256, 1024, 1024, 9, 0, 16, 16, 0, 1), (4, 7, "igemm4_halo_kernel<16, 6>")),
    "halo tiles over two-team": ((4096, 512, 256, 9, 0, 64, 64, 0, 1), (1, 7, "igemm4_halo_kernel<64, 6>")),
    "tall 128x64 tiles": ((4096, 512, 512, 9, 0, 64, 64, 0, 1), (1, 12, "igemm4_kernel<128, 64, 64, 6, 3, 1>")),
    "igemm4 two-team (chunks do not split evenly)": ((1024, 1344, 512, 9, 0, 32, 32, 0, 1), (2, 10, "igemm4_kernel<64, 64, 32, 6, 3, 2>")),
    "4-slot ring: 12-step slices": ((256, 512, 512, 9, 0, 16, 16, 1, 0), (8, 9, "igemm4_kernel<64, 64, 16, 4, 3, 1>")),
    "6-slot ring: 27-step slices": ((256, 1536, 768, 9, 0, 16, 16, 0, 1), (8, 9, "igemm4_kernel<64, 64, 16, 6, 3, 1>")),
    "1x1 64-tile, M = 256": ((256, 1024, 1024, 1, 0, 16, 16, 0, 0), (1, 3, "igemm2_kernel<64, 64, 4, false, 1>")),
}

_IG2_1 = (1, "igemm2_kernel<64, 64, 4, true, 1>")
_IG2_2 = (4, "igemm2_kernel<64, 64, 4, true, 2>")


def _k(ks, route):
    return (ks,) + route


# switch -> the cases whose choice it changes, and their choice under it (every other case keeps its default)
SWITCHES = {
    "ISHAP_IGEMM4=0": {
        "3x3 on an 8x8 map, small-map slices": _k(16, _IG2_1),
        "3x3 on an 8x8 map, folded source": _k(16, _IG2_1),
        "3x3 on an 8x8 map, generic split": _k(16, _IG2_1),
        "3x3 128-tile": (1, 0, "igemm2_kernel<128, 128, 4, true, 1>"),
        "3x3 128-tile, folded source": (1, 0, "igemm2_kernel<128, 128, 4, true, 1>"),
        "halo tiles 64^2": _k(1, _IG2_2),
        "halo tiles 32^2, 2 slices": _k(2, _IG2_2),
        "halo tiles 16^2, 4 slices": _k(4, _IG2_2),
        "halo tiles over two-team": _k(1, _IG2_2),
        "tall 128x64 tiles": _k(1, _IG2_1),
        "igemm4 two-team (chunks do not split evenly)": _k(2, _IG2_2),
        "4-slot ring: 12-step slices": _k(8, _IG2_1),
        "6-slot ring: 27-step slices": _k(8, _IG2_1),
    },
    "ISHAP_IGEMM4=1": {     # igemm4's 128x128 tiles only, and no small-map slices
        "3x3 on an 8x8 map, small-map slices": _k(16, _IG2_1),
        "3x3 on an 8x8 map, folded source": _k(16, _IG2_1),
        "3x3 on an 8x8 map, generic split": _k(16, _IG2_1),
        "halo tiles 64^2": _k(1, _IG2_2),
        "halo tiles 32^2, 2 slices": _k(2, _IG2_2),
        "halo tiles 16^2, 4 slices": _k(4, _IG2_2),
        "halo tiles over two-team": _k(1, _IG2_2),
        "tall 128x64 tiles": _k(1, _IG2_1),
        "igemm4 two-team (chunks do not split evenly)": _k(2, _IG2_2),
        "4-slot ring: 12-step slices": _k(8, _IG2_1),
        "6-slot ring: 27-step slices": _k(8, _IG2_1),
    },
    "ISHAP_IG4_TEAMS=0": {
        "tall 128x64 tiles": (1, 9, "igemm4_kernel<64, 64, 64, 6, 3, 1>"),
        "igemm4 two-team (chunks do not split evenly)": (2, 9, "igemm4_kernel<64, 64, 32, 6, 3, 1>"),
    },
    "ISHAP_IG4_TEAMS=1": {  # tall tiles on, two teams off
        "igemm4 two-team (chunks do not split evenly)": (2, 9, "igemm4_kernel<64, 64, 32, 6, 3, 1>"),
    },
    "ISHAP_IG4_HALO=0": {
        "halo tiles 64^2": (1, 9, "igemm4_kernel<64, 64, 64, 6, 3, 1>"),
        "halo tiles 32^2, 2 slices": (2, 9, "igemm4_kernel<64, 64, 32, 6, 3, 1>"),
        "halo tiles 16^2, 4 slices": (4, 9, "igemm4_kernel<64, 64, 16, 6, 3, 1>"),
        "halo tiles over two-team": (1, 10, "igemm4_kernel<64, 64, 64, 6, 3, 2>"),
    },
    "ISHAP_HALVES=1": {
        "3x3 64-tile, folded source: igemm2 two-team": _k(2, _IG2_1),
    },
    "ISHAP_SKINNY=0": {
        "skinny 1x1 on an 8x8 map": (1, 3, "igemm2_kernel<64, 64, 4, false, 1>"),
        "skinny 1x1, pending but K < 2048": (1, 3, "igemm2_kernel<64, 64, 4, false, 1>"),
    },
    "ISHAP_G1_SLICES=0": {
        "sliced 1x1, K = 3072": (1, 5, "igemm_skinny_kernel<2, false>"),
        "sliced 1x1, K = 2048": (1, 5, "igemm_skinny_kernel<2, false>"),
    },
    "ISHAP_BIG_MIN=1": {
        "3x3 64-tile, folded source: igemm2": (2, 8, "igemm4_kernel<128, 128, 64, 5, 3, 1>"),
        "3x3 64-tile, folded source: igemm2 two-team": (8, 8, "igemm4_kernel<128, 128, 32, 5, 3, 1>"),
        "halo tiles 64^2": (4, 8, "igemm4_kernel<128, 128, 64, 5, 3, 1>"),
        "halo tiles 32^2, 2 slices": (8, 8, "igemm4_kernel<128, 128, 32, 5, 3, 1>"),
        "halo tiles 16^2, 4 slices": (16, 8, "igemm4_kernel<128, 128, 16, 5, 3, 1>"),
        "halo tiles over two-team": (4, 8, "igemm4_kernel<128, 128, 64, 5, 3, 1>"),
        "tall 128x64 tiles": (2, 8, "igemm4_kernel<128, 128, 64, 5, 3, 1>"),
        "igemm4 two-team (chunks do not split evenly)": (8, 8, "igemm4_kernel<128, 128, 32, 5, 3, 1>"),
        "4-slot ring: 12-step slices": (16, 8, "igemm4_kernel<128, 128, 16, 5, 3, 1>"),
        "6-slot ring: 27-step slices": (32, 8, "igemm4_kernel<128, 128, 16, 5, 3, 1>"),
        "1x1 64-tile, M = 256": (1, 2, "igemm2_kernel<128, 128, 4, false, 1>"),
    },
}

# run in a child process (the switches are read once per process): every case's plan as JSON
_CHILD = f"""
import ctypes as C, json, sys
sys.path.insert(0, {ROOT!r})
from ishapediting_amd import _lib
L = _lib.lib()
out = {{}}
for name, args in json.loads(sys.argv[1]).items():
    ks, slot, kern = C.c_int(), C.c_int(), C.create_string_buffer(96)
    M, cin, cout, taps, k2, h, w, pending, sums = args
    rc = L.ishap_igemm_plan(M, cin, cout, taps, k2, h, w, 1, pending, sums, C.byref(ks), C.byref(slot), kern, len(kern))
    out[name] = [ks.value, slot.value, kern.value.decode()] if rc == 0 else rc
print(json.dumps(out))
"""


def _plans(envs):
    """{env setting: {case: plan}}, one child process per setting, all at once"""
    cases = json.dumps({n: list(a) for n, (a, _) in CASES.items()})
    procs = {}
    for e in envs:
        env = {k: v for k, v in os.environ.items() if not k.startswith("ISHAP_")}
        if e:
            k, v = e.split("=")
            env[k] = v
        procs[e] = subprocess.Popen([sys.executable, "-c", _CHILD, cases], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                    text=True)
    res = {}
    for e, p in procs.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-2000:]
        res[e] = {n: tuple(v) if isinstance(v, list) else v for n, v in json.loads(out.strip().splitlines()[-1]).items()}
    return res


@pytest.fixture(scope="module")
def plans():
    return _plans([""] + list(SWITCHES))


def test_every_rule_picks_the_kernel_it_picked_before(plans):
    got = plans[""]
    bad = {n: (got[n], exp) for n, (_, exp) in CASES.items() if got[n] != exp}
    assert not bad, bad
    assert {exp[1] for _, exp in CASES.values()} == set(range(13))      # every profiling slot is reached


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_each_switch_changes_the_route_it_documents(plans, switch):
    want = {n: SWITCHES[switch].get(n, exp) for n, (_, exp) in CASES.items()}
    got = plans[switch]
    bad = {n: (got[n], want[n]) for n in CASES if got[n] != want[n]}
    assert not bad, bad


def test_plan_reports_a_short_name_buffer():
    from ishapediting_amd import _lib
    L = _lib.lib()
    ks, slot, kern = C.c_int(), C.c_int(), C.create_string_buffer(8)
    assert L.ishap_igemm_plan(4096, 256, 256, 9, 0, 64, 64, 1, 0, 0, C.byref(ks), C.byref(slot), kern, len(kern)) == -2
