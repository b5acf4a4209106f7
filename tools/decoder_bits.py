"""One sha256 per output of the fp32-MFMA triplane decoder kernels (csrc/decode_mlp.h: triplane_field_kernel,
triplane_project_kernel, triplane_fit_kernel) on fixed seeded inputs, to compare two builds of the library bit for bit.

  * field / projection (no atomics, repeatable): S in {2, 128} x npts in {1, 33, 1061} -- a lone point, a tail tile, more
    tiles than one workgroup's four waves -- coordinates uniform in [-1.2, 1.2]^3 so that border cells and zero padding
    occur; ishap_triplane_field_grad (logits, grad) and ishap_triplane_project with 0 and 4 iterations (x_out, logits,
    normals, accepted).
  * fit (float atomics, so hashed only where their order cannot matter): S = 128, a single tile per launch,
    (nbatch, nrand) = (32, 0), (17, 0), (0, 32); each of the 32 points takes x, y and z from 32 values spaced 4 texels
    apart, permuted per axis, and the pair noise is clamped to [-1, 1].  Before a launch the tool asserts on the host that
    no plane texel is tapped by two different points (or two different pairs): every address then receives one add, or the
    two commuting adds of a pair, and loss_parts one add from one wave (the idle waves add +0).

Run it once per library, each in a fresh process, and diff the outputs.
Usage: python tools/decoder_bits.py [--lib path/to/libishap_hip.so]"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def report(case, **outs):
    for name, t in outs.items():
        print(f"{case:28s} {name:9s} {sha(t)}")


def tapped_texels(pts, S):
    """per point the set of (plane, y, x) its bilinear cells touch: the kernels' fp32 arithmetic (mlp_cell) on the host"""
    pts = np.asarray(pts, np.float32)
    half, sm1 = np.float32(2), np.float32(S - 1)
    out = []
    for c in pts:
        s = set()
        for p, (u, v) in enumerate(((c[0], c[1]), (c[1], c[2]), (c[0], c[2]))):
            x0 = int(np.floor(((u + np.float32(1)) / half) * sm1))
            y0 = int(np.floor(((v + np.float32(1)) / half) * sm1))
            s |= {(p, y, x) for y in (y0, y0 + 1) for x in (x0, x0 + 1) if 0 <= x < S and 0 <= y < S}
        out.append(s)
    return out


def assert_disjoint(groups):
    """groups: per work item (a point, or a pair) its set of texels"""
    seen = {}
    for i, s in enumerate(groups):
        for t in s:
            assert seen.setdefault(t, i) == i, f"texel {t} is tapped by items {seen[t]} and {i}: the atomics' order would matter"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the library to load instead of the installed one")
    a = ap.parse_args()
    from ishapediting_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from ishapediting_amd import synthetic
    from ishapediting_amd.triplane_decoder import MultiTriplane, field_grad_planes, project_to_surface
    dev = torch.device("cuda", 0)
    dec = MultiTriplane(1, device=dev)
    dec.net.load_state_dict(synthetic.decoder_state_dict(4321))

    for S in (2, 128):
        g = torch.Generator().manual_seed(100 + S)
        planes = (torch.randn(3, S, S, 32, generator=g) * 0.3).to(dev)
        for n in (1, 33, 1061):
            pts = ((torch.rand(n, 3, generator=g) * 2 - 1) * 1.2).to(dev)
            f = field_grad_planes(dec, planes, pts)
            report(f"field S={S} n={n}", logits=f.logits, grad=f.grad)
            for it in (0, 4):
                p = project_to_surface(dec, planes, pts, iterations=it)
                report(f"project S={S} n={n} it={it}", x_out=p.points, logits=p.logits, normals=p.normals, accepted=p.accepted)

    S = 128
    g = torch.Generator().manual_seed(7)
    planes = (torch.randn(3, S, S, 32, generator=g) * 0.3).to(dev)
    texel = 2.3 + 4.0 * torch.arange(32, dtype=torch.float64)            # cells 2 + 4k; a pair partner stays within a texel
    axis = (2.0 * texel / (S - 1) - 1.0).float()
    coords = torch.stack([axis[torch.randperm(32, generator=g)] for _ in range(3)], dim=1)
    gt = (torch.rand(32, generator=g) < 0.5).float()
    idx = torch.randperm(32, generator=g).to(torch.int32)
    noise = torch.randn(32, 3, generator=g).clamp(-1.0, 1.0)
    partner = coords + noise * 0.01                                      # fp32 mul, then add: as fit_point
    empty = torch.zeros(0, 3)
    for nbatch, nrand in ((32, 0), (17, 0), (0, 32)):
        if nrand:
            ta, tb = tapped_texels(coords[:nrand], S), tapped_texels(partner[:nrand], S)
            assert_disjoint([x | y for x, y in zip(ta, tb)])
        else:
            assert_disjoint(tapped_texels(coords[idx[:nbatch].long()], S))
        loss_parts, dplanes = dec.fit_loss_grad(planes, coords, gt, idx[:nbatch], coords[:nrand] if nrand else empty,
                                                noise[:nrand] if nrand else empty)
        torch.cuda.synchronize()
        report(f"fit b={nbatch} r={nrand}", loss=loss_parts, dplanes=dplanes)


if __name__ == "__main__":
    main()
