"""The 128-pixel x 32-channel halo tiles of the 3x3 convolution (csrc/igemm4.hip igemm4_halo_kernel) against the tile forms
they replace (ISHAP_IG4_HALO=0), on the full-size model: forward output, the 64^2 x 512 tap, and the input gradient of a guided
step, each build in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_fullsize import rel

pytestmark = pytest.mark.gpu

_WORKER = r"""
import sys, ctypes as C, numpy as np, torch
sys.path.insert(0, {root!r})
from ishapediting_amd import synthetic, _lib
from ishapediting_amd.unet import UNetModel
from ishapediting_amd.unet_spec import full_config
cfg = full_config()
dev = torch.device("cuda", 0)
m = UNetModel(cfg, dev)
m.load_state_dict(synthetic.round_torso_to_fp16(synthetic.unet_state_dict(cfg, 1234)))
x = torch.from_numpy(synthetic.latent(2)).to(dev)
k = 8
ch, sz = m.tap_shape(k)
cot = (torch.randn(1, sz * sz, ch, generator=torch.Generator().manual_seed(3)) * 1e-2).half().to(dev)
L = _lib.lib()
L.ishap_profile_begin()
out, tap = m(x, [617.0], feat_layer=k, keep_for_backward=True)
gx = m.backward_input(cot)
torch.cuda.synchronize()
buf = (C.c_double * 39)()
assert L.ishap_profile_end(buf, 13) == 0
assert int(L.ishap_device_status()) == 0
np.savez({out!r}, out=out.cpu().numpy(), tap=tap.float().cpu().numpy(), gx=gx.cpu().numpy(), launches=np.array([buf[v * 3] for v in range(13)]))
"""

HALO_VARIANT = 7      # igemm.hip ishap_profile_end: the halo tiles' slot


def _run(tmp_path, name, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / (name + ".npz"))
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _WORKER.format(root=root, out=path)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, r.stderr[-2000:])
    return np.load(path)


def test_halo_tiles_match_the_tiles_they_replace(tmp_path):
    """The halo tiles keep K in the one-team 64x64 kernel's order (chunk, dy, dx, K half), so a launch with the same K partition
    stores the same bits; the layers that move from the two-team form (its K halves meet in the epilogue) change the summation
    order, and the fixed-point GroupNorm statistics are summed over 128-pixel tiles instead of 64: the same relative bounds as
    test_gpu_fullsize.py's igemm4 / igemm2 comparison (2e-3 forward, 5e-3 gradient)."""
    new = _run(tmp_path, "halo", {})
    old = _run(tmp_path, "nohalo", {"ISHAP_IG4_HALO": "0"})
    # the switch selects the kernel: launches of the halo form only with it on
    assert new["launches"][HALO_VARIANT] > 0 and old["launches"][HALO_VARIANT] == 0, (new["launches"], old["launches"])
    errs = {k: rel(torch.from_numpy(new[k]), torch.from_numpy(old[k])) for k in ("out", "tap", "gx")}
    print("halo vs ISHAP_IG4_HALO=0: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert errs["out"] < 2e-3 and errs["tap"] < 2e-3 and errs["gx"] < 5e-3, errs
    assert np.isfinite(new["out"]).all() and np.isfinite(new["gx"]).all()
