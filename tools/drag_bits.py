"""One sha256 per output of the drag loss kernels on fixed inputs, to compare two builds of the library bit for bit:
gradient, loss, cotangent, scale2 and the touched bitmap of
  * one edit (DragKernels: ishap_drag_batch_setup / _loss_cotangent with E = 1) on the four G7 cases (l2 / l1, cof 0 / 0.4;
    tests/golden/g7_drag.npz),
  * a batch on the E = 3 case of tests/test_gpu_batched_drag.py (1, 3 and 2 handles, cof 0 / 0.2 / 0.4, own guidance),
  * one edit at full size (W = 64, ld = 512, feat_channel_map(512), DragStuff's r1 = 12 and voxel = 2 / 256, three seeded
    handles, seeded fp16 taps, cof 0.2).
Run it once per installed library and diff the outputs.  Usage: python tools/drag_bits.py"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def report(case, grad, loss, cot, scale2, touched):
    for name, t in (("gradient", grad), ("loss", loss), ("cotangent", cot), ("scale2", scale2), ("touched", touched)):
        print(f"{case:28s} {name:9s} {sha(t)}")


def _tap_from_planes(feat):
    """[3,Cc,W,W] fp32 -> NHWC fp16 tap [W*W][ld] + chmap (plane p channel c at p*Cc+c), as the drag tests build it."""
    P, Cc, W, _ = feat.shape
    ld = ((P * Cc + 31) // 32) * 32
    tap = torch.zeros(W * W, ld, dtype=torch.float16)
    tap[:, :P * Cc] = feat.reshape(P * Cc, W * W).t().half()
    return tap, torch.arange(P * Cc, dtype=torch.int32).reshape(P, Cc), ld


def solo(case, dev, W, ld, chmap, r, voxel, loss_type, src, tgt, cof, edit, orig):
    from ishapediting_amd.drag_utils import DragKernels
    dk = DragKernels(dev, W=W, ld=ld, chmap=chmap, r=r, voxel=voxel, loss_type=loss_type)
    dk.setup(src, tgt, cof)
    e_d, o_d = edit.to(dev).contiguous(), orig.to(dev).contiguous()
    cot, sc = dk.loss_cotangent_ptr(e_d.data_ptr(), o_d.data_ptr())
    torch.cuda.synchronize()
    report(case, dk.grad, dk.loss, cot, sc, dk.touched)


def main():
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import BatchDragKernels, feat_channel_map
    dev = torch.device("cuda", 0)
    T = torch.from_numpy
    g = np.load(os.path.join(ROOT, "tests", "golden", "g7_drag.npz"))
    base_e, chmap, ld = _tap_from_planes(T(g["edit"]))
    base_o, _, _ = _tap_from_planes(T(g["orig"]))
    W, r, voxel = 16, int(g["r1"]), float(g["voxel_size"])
    for lt in ("l2", "l1"):
        for cof in (0.0, 0.4):
            solo(f"g7 solo {lt} cof {cof}", dev, W, ld, chmap, r, voxel, lt, g["sources"], g["targets"], cof, base_e, base_o)
    # the E = 3 case of test_batched_drag_loss_is_bitwise_the_solo_loss (shared = False), same generator and draw order
    for lt in ("l2", "l1"):
        gen = torch.Generator().manual_seed(11)
        E, nh, cofs = 3, [1, 3, 2], [0.0, 0.2, 0.4]
        edits = torch.stack([(base_e.float() + 0.05 * e * torch.randn(base_e.shape, generator=gen)).half() for e in range(E)])
        origs = torch.stack([(base_o.float() + 0.05 * e * torch.randn(base_o.shape, generator=gen)).half() for e in range(E)])
        srcs = [(torch.rand(n, 3, generator=gen) * 1.6 - 0.8) for n in nh]
        tgts = [s + (torch.rand(s.shape, generator=gen) - 0.5) * 0.4 for s in srcs]
        bk = BatchDragKernels(dev, E, W=W, ld=ld, chmap=chmap, r=r, voxel=voxel, loss_type=lt)
        bk.setup(srcs, tgts, cofs)
        e_d, o_d = edits.to(dev).contiguous(), origs.to(dev).contiguous()
        cot, sc = bk.loss_cotangent_ptr(e_d.data_ptr(), o_d.data_ptr(), W * W * ld)
        torch.cuda.synchronize()
        report(f"batch E=3 {lt}", bk.grad, bk.loss, cot, sc, bk.scratch_parts()["touched"])
    # full size
    W, ld = 64, 512
    gen = torch.Generator().manual_seed(23)
    edit = (torch.randn(W * W, ld, generator=gen) * 0.5).half()
    orig = (edit.float() + 0.1 * torch.randn(W * W, ld, generator=gen)).half()
    src, tgt = synthetic.handles(3, seed=7)
    solo("full size solo l2 cof 0.2", dev, W, ld, feat_channel_map(ld), 12, 2.0 / 256, "l2", src, tgt, 0.2, edit, orig)


if __name__ == "__main__":
    main()
