#!/usr/bin/env python3
"""Golden G17: ten train_triplane_opt steps (drag_utils.py:521-539) run by the REFERENCE's own MultiTriplane
(triplane_decoder/axisnetworks.py: forward, l2reg, tvreg) and torch.optim.Adam, on the CPU in fp32.

Inputs: synthetic decoder weights (ishapediting_amd.synthetic.decoder_state_dict, stored as seed + checksum), S = 32 planes
init as randn * stds + means, 8 000 occupancy samples of a sphere, ten injected batches (idx, r, noise) of 1 000.  Every
input is rounded to fp16 so that it is stored exactly in half the bytes; the fixture holds the inputs, the step-1 loss
parts and gradient (embeddings[i].grad) and the ten per-step losses.  Run here once; the tests read only the .npz.

    python tools/make_triplane_opt_fixture.py --reference DIR [--out tests/golden/g17_triplane_opt.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, P, STEPS, BATCH, DEC_SEED, SEED = 32, 8000, 10, 1000, 4321, 17


def f16(t):
    return t.half().float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds triplane_decoder/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g17_triplane_opt.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from triplane_decoder.axisnetworks import MultiTriplane
    from ishapediting_amd import synthetic
    import torch.nn.functional as ff

    torch.manual_seed(SEED)
    sd = synthetic.decoder_state_dict(DEC_SEED)
    dec = MultiTriplane(1, input_dim=3, output_dim=1, device="cpu")
    dec.net.load_state_dict(sd)
    means = 0.05 * torch.randn(96)
    stds = 0.3 + 0.2 * torch.rand(96)
    planes0 = f16(torch.randn(1, 96, S, S) * stds.reshape(1, 96, 1, 1) + means.reshape(1, 96, 1, 1)).reshape(3, 32, S, S)
    uni = torch.rand(P // 2, 3) * 2 - 1
    d = torch.randn(P - P // 2, 3)
    surf = 0.6 * d / d.norm(dim=1, keepdim=True) + 0.01 * torch.randn(P - P // 2, 3)
    coords = f16(torch.cat([uni, surf]))
    gt = (coords.norm(dim=1) < 0.6).float()
    idx = torch.stack([torch.randperm(P)[:BATCH] for _ in range(STEPS)])
    r = f16(torch.rand(STEPS, BATCH, 3) * 2 - 1)
    noise = f16(torch.randn(STEPS, BATCH, 3))

    for i in range(3):
        dec.embeddings[i] = planes0[[i]].clone().requires_grad_(True)
    opt = torch.optim.Adam(params=dec.embeddings, lr=0.001, betas=(0.9, 0.999))
    parts, grad1 = [], None
    for k in range(STEPS):       # drag_utils.py:526-539 with the batch, rand_coord and randn_like injected
        coord, g = coords[idx[k]], gt[idx[k]].reshape(-1, 1)
        prediction = dec(0, coord.unsqueeze(0)).squeeze(0)
        bce = torch.nn.BCEWithLogitsLoss()(prediction, g)
        rand_coord = r[k]
        rand_coord_offset = rand_coord + noise[k] * 1e-2
        mse = ff.mse_loss(dec(0, rand_coord.unsqueeze(0)).squeeze(0), dec(0, rand_coord_offset.unsqueeze(0)).squeeze(0))
        l2, tv = dec.l2reg(), dec.tvreg()
        loss = bce + mse * 0.3 + l2 * 0.001 + tv * 0.01
        loss.backward()
        if grad1 is None:
            grad1 = torch.cat([e.grad.detach().clone() for e in dec.embeddings])
        opt.step()
        opt.zero_grad()
        parts.append([float(bce), float(mse), float(l2), float(tv), float(loss)])
        print(k, parts[-1])
    dec_check = sum(float(v.double().abs().sum()) for v in sd.values())
    np.savez_compressed(
        a.out, S=S, dec_seed=DEC_SEED, dec_check=dec_check, planes0=planes0.half().numpy(), coords=coords.half().numpy(),
        gt=gt.to(torch.uint8).numpy(), idx=idx.to(torch.int16).numpy(), r=r.half().numpy(), noise=noise.half().numpy(),
        parts=np.array(parts, np.float64), grad1=grad1.numpy().astype(np.float32))
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
