"""The volume-constraint loss (csrc/constrain.hip) restated in float64 on tests/decoder_ref.py's machinery, and its gather list
in numpy.

  L_vol = -(1 / Wsum) sum_j w_j BCEWithLogits(decoder(planes)(q_j), g_j),  Wsum = sum_j w_j (in double).

weighted_loss_grad returns what decoder_ref.points_loss_grad returns -- loss, dplanes, logits, the magnitude scatters A, A1,
Aw and the tap counts cnt -- with the weights carried through, so that decoder_ref.measured_rel, derived_terms and
backward_bound apply unchanged:
  A    sum |w_q| |d L / d feature|: the weights sit inside d L / d feature;
  A1   the scatter of d (sum_j w_j z_j / Wsum) / d features: the kernel's rounded sigmoid is an absolute error of a few u in
       sigmoid - g, which the point's w_j / Wsum then scales (for w = 1 this is d (mean z) / d features, exactly);
  cnt  derived_terms charges cnt u A for cnt float atomics in any order; the gather pass adds the same cnt products in a fixed
       order, fewer than cnt roundings of partial sums no larger than A: the same term.
  bce_abs_mean = sum_j w_j |bce_j| / Wsum, the size the loss bound 2^-20 (1 + bce_abs_mean) is relative to.
With w = 1 everywhere every returned number equals points_loss_grad's exactly (w z = z and Wsum = float(n) in float64).

gather_list states ishap_constraint_setup: the kernel's fp32 tap arithmetic (decoder_ref.taps in float32 is mlp_cell's order),
out-of-range taps dropped, entries grouped by texel row and ascending by 4 j + q within a row.
"""
from types import SimpleNamespace

import numpy as np
import torch

from tests import decoder_ref as D


def weighted_loss_grad(net, planes, coords, gt, w, dtype=torch.float64):
    planes = np.asarray(planes)
    S = planes.shape[1]
    P = torch.as_tensor(planes.reshape(-1, 32).astype(np.float64)).to(dtype).requires_grad_(True)
    rec = []
    z = D._decode_t(D._net_t(net, dtype), P, coords, S, dtype, rec)
    wt = torch.as_tensor(np.asarray(w, np.float64)).to(dtype)
    wsum = float(np.asarray(w, np.float64).sum())
    assert wsum > 0
    bce = D._bce(z, torch.as_tensor(np.asarray(gt, np.float64)).to(dtype))
    loss = -(wt * bce).sum() / wsum
    f = rec[0][2]
    dzdf, = torch.autograd.grad((wt * z).sum() / wsum, f, retain_graph=True)
    dldf, = torch.autograd.grad(loss, f, retain_graph=True)
    gP, = torch.autograd.grad(loss, P)
    sc = lambda g, **kw: D._scatter_abs(rec, 3 * S * S, [g], **kw).reshape(planes.shape)      # noqa: E731
    return SimpleNamespace(loss=float(loss.detach()), dplanes=gP.double().numpy().reshape(planes.shape), logits=z.detach().double().numpy(),
                           bce_abs_mean=float((wt * bce.detach().abs()).sum() / wsum), A=sc(dldf), A1=sc(dzdf), Aw=sc(dldf, weights_error=True),
                           cnt=sc(dldf, count=True))


def gather_list(coords, S):
    """-> row_start int32 [3 S S + 1], entry int32 [n], entry_w float32 [n] of fp32 coords [M, 3]"""
    t = D.taps(np.asarray(coords, np.float32), S, np.float32)
    M = t.tex.shape[0]
    key = (4 * np.arange(M, dtype=np.int64)[:, None, None] + np.arange(4, dtype=np.int64)[None, None, :]) + np.zeros((1, 3, 1), np.int64)
    ok = t.tex >= 0
    rows, keys, ws = t.tex[ok], key[ok], t.w[ok].astype(np.float32)
    order = np.lexsort((keys, rows))
    row_start = np.zeros(3 * S * S + 1, np.int64)
    row_start[1:] = np.cumsum(np.bincount(rows, minlength=3 * S * S))
    return row_start.astype(np.int32), keys[order].astype(np.int32), ws[order]
