"""Test-side statement of one train_triplane_opt step (drag_utils.py:521-539) in plain torch autograd, in fp32 or fp64.

Planes are [3,32,S,S] (the reference's three embeddings, stacked); the decoder is oracle.ref_cpu.decoder_forward."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.ref_cpu import decoder_forward

PAIR_W, L2_W, TV_W = 0.3, 0.001, 0.01

# Spreads between an fp32 and an fp64 run of triplane_opt_ref on golden G17's inputs, measured on the CPU
# (tests/triplane_opt_ref.run_fit in both precisions).  The fp32 run reproduces the fixture bit for bit.
G17_TOTAL_LOSS_SPREAD = 1.51e-5        # max over the ten steps of |total_fp32 - total_fp64|
G17_GRAD1_SPREAD = 1.09e-3             # relative L2 of the step-1 gradient (the pair mse's z_r - z_r+delta cancels)
G17_DISPLACEMENT_SPREAD = 1.10e-2      # relative L2 of the planes' displacement after ten steps (Adam's first steps
                                       # are sign-like: last-bit differences of small gradients become lr-sized moves)


def net_as(net, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in net.items()}


def l2reg(planes):
    return sum((planes[p] ** 2).sum() ** 0.5 for p in range(3))


def tvreg(planes):
    l = 0
    for p in range(3):
        e = planes[p]
        l = l + ((e[:, 1:] - e[:, :-1]) ** 2).sum() ** 0.5 + ((e[:, :, 1:] - e[:, :, :-1]) ** 2).sum() ** 0.5
    return l


def data_pair_terms(net, planes, coords, gt, idx, r, noise):
    """(bce, mse) of one step: BCEWithLogits on coords[idx], mse between r and r + 0.01 * noise."""
    idx = torch.as_tensor(np.asarray(idx)).long()
    z = decoder_forward(net, planes, coords[idx])
    bce = F.binary_cross_entropy_with_logits(z, gt[idx])
    ro = r + noise * 1e-2
    mse = F.mse_loss(decoder_forward(net, planes, r), decoder_forward(net, planes, ro))
    return bce, mse


def step_loss(net, planes, coords, gt, idx, r, noise):
    """-> (parts [bce, mse, l2, tv], total), differentiable in planes."""
    bce, mse = data_pair_terms(net, planes, coords, gt, idx, r, noise)
    l2, tv = l2reg(planes), tvreg(planes)
    return torch.stack([bce, mse, l2, tv]), bce + PAIR_W * mse + L2_W * l2 + TV_W * tv


def run_fit(net, planes0, coords, gt, batches, dtype=torch.float64, lr=1e-3):
    """Adam over the injected batches [(idx, r, noise), ...].  Returns (losses [steps,4], totals [steps], planes,
    step-1 gradient), all in `dtype`."""
    net = net_as(net, dtype)
    p = torch.as_tensor(np.asarray(planes0)).to(dtype).clone().requires_grad_(True)
    coords = torch.as_tensor(np.asarray(coords)).to(dtype)
    gt = torch.as_tensor(np.asarray(gt)).to(dtype).reshape(-1)
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    losses, totals, grad1 = [], [], None
    for idx, r, noise in batches:
        parts, total = step_loss(net, p, coords, gt, idx, torch.as_tensor(np.asarray(r)).to(dtype),
                                 torch.as_tensor(np.asarray(noise)).to(dtype))
        opt.zero_grad()
        total.backward()
        if grad1 is None:
            grad1 = p.grad.detach().clone()
        opt.step()
        losses.append(parts.detach())
        totals.append(total.detach())
    return torch.stack(losses), torch.stack(totals), p.detach(), grad1


def fixture_batches(g):
    """The injected (idx, r, noise) of golden G17, as float32 / int64 arrays."""
    return [(g["idx"][k].astype(np.int64), g["r"][k].astype(np.float32), g["noise"][k].astype(np.float32))
            for k in range(g["idx"].shape[0])]


def fixture_inputs(g):
    """(net, planes0 [3,32,S,S], coords [P,3], gt [P]) of golden G17 as float32; the decoder weights are
    synthetic.decoder_state_dict(seed), checked against the stored checksum."""
    from ishapediting_amd import synthetic
    net = {k: v.numpy() for k, v in synthetic.decoder_state_dict(int(g["dec_seed"])).items()}
    chk = sum(float(np.abs(v.astype(np.float64)).sum()) for v in net.values())
    np.testing.assert_allclose(chk, float(g["dec_check"]), rtol=1e-12, err_msg="synthetic decoder weights differ from the fixture's")
    return net, g["planes0"].astype(np.float32), g["coords"].astype(np.float32), g["gt"].astype(np.float32)
