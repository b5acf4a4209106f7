"""QKVAttentionLegacy (gd/unet.py:337-354, oracle/ref_cpu.py attention) in float64, for tests/test_gpu_attention_oracle.py.

Layout: a token row of qkv holds 3C values; head h sits at channels [h*3d, (h+1)*3d) as q | k | v, and a = softmax(alpha q k^T) v
with alpha = 1/sqrt(d) (the legacy form scales q and k by d^-1/4 each).  Tensors are [N][T][3C] (qkv), [N][T][C] (a, dA) and
[N*heads][T] (lse), the layouts of csrc/attention.hip.

Three things live here:
  * statement(): the operation itself, per (image, head) chunk so that T = 1024, N = 8 stays small, with the float64 autograd
    gradients dq, dk, dv;
  * magnitudes(): the sums of magnitudes the test's error bounds are stated in (test_gpu_attention_oracle.py docstring);
  * restatement(): the same attention walked as the kernels walk it -- 64-key tiles, team t takes tiles t, t + TEAMS, ...,
    an online softmax per team, the teams merged in team order; the backward with two teams over alternating tiles whose sums
    are added.  Its switches are the kernel bugs the bounds must catch (test_bounds_reject_mutated_references)."""
import math

import torch

TILE = 64


def split_heads(qkv, heads, d, layout="qkv"):
    """[N][T][3C] -> q, k, v as float64 [N][heads][T][d]; layout "kqv": a launcher that took k for q and q for k"""
    N, T, _ = qkv.shape
    x = qkv.double().reshape(N, T, heads, 3, d).permute(3, 0, 2, 1, 4)
    q, k, v = x[0], x[1], x[2]
    if layout == "kqv":
        q, k = k, q
    return q, k, v


def merge_heads(t):
    """[N][heads][T][d] -> [N][T][heads * d]"""
    N, H, T, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(N, T, H * d)


def statement(qkv, heads, d, dA=None):
    """float64 attention of the fp16 qkv: a [N][T][C], lse [N*heads][T]; with dA [N][T][C] also dqkv [N][T][3C] by autograd"""
    N, T, _ = qkv.shape
    C = heads * d
    q, k, v = split_heads(qkv, heads, d)
    a = torch.empty(N, heads, T, d, dtype=torch.float64)
    lse = torch.empty(N, heads, T, dtype=torch.float64)
    grads = torch.zeros(3, N, heads, T, d, dtype=torch.float64) if dA is not None else None
    gA = dA.double().reshape(N, T, heads, d).permute(0, 2, 1, 3) if dA is not None else None
    s = 1.0 / math.sqrt(math.sqrt(d))
    for n in range(N):
        for h in range(heads):
            qq, kk, vv = (t[n, h].clone().requires_grad_(dA is not None) for t in (q, k, v))
            with torch.set_grad_enabled(dA is not None):
                w = torch.einsum("tc,sc->ts", qq * s, kk * s)
                lse[n, h] = torch.logsumexp(w.detach(), -1)
                o = torch.softmax(w, dim=-1) @ vv
                if dA is not None:
                    o.backward(gA[n, h])
                    grads[0, n, h], grads[1, n, h], grads[2, n, h] = qq.grad, kk.grad, vv.grad
            a[n, h] = o.detach()
    out = merge_heads(a), lse.reshape(N * heads, T)
    if dA is None:
        return out
    dqkv = torch.stack([grads[0], grads[1], grads[2]], 3)          # [N][heads][T][3][d]
    return out + (dqkv.permute(0, 2, 1, 3, 4).reshape(N, T, 3 * C),)


def magnitudes(qkv, heads, d, dA=None, a=None):
    """The magnitude sums the bounds use, float64:
       forward  E [N*heads][T] = d 2^-24 max_k S_abs + 2^-20 with S_abs = alpha sum_d |q_d k_d|, and V1 [N][T][C] = sum_k w_k |v_k|;
       backward (dA and the exact a given) G [N][T][3C]: for dq sum_k alpha P (dP_abs + D_abs) |k|, for dk the same over queries
       with |q|, for dv sum_q P |dA|, where dP_abs = |dA| |v|^T and D_abs = sum_d |dA| |a|."""
    N, T, _ = qkv.shape
    alpha = 1.0 / math.sqrt(d)
    q, k, v = split_heads(qkv, heads, d)
    E = torch.empty(N, heads, T, dtype=torch.float64)
    V1 = torch.empty(N, heads, T, d, dtype=torch.float64)
    G = torch.zeros(N, heads, T, 3, d, dtype=torch.float64) if dA is not None else None
    if dA is not None:
        gA = dA.double().reshape(N, T, heads, d).permute(0, 2, 1, 3)
        aa = a.double().reshape(N, T, heads, d).permute(0, 2, 1, 3)
    for n in range(N):
        for h in range(heads):
            qq, kk, vv = q[n, h], k[n, h], v[n, h]
            sabs = alpha * (qq.abs() @ kk.abs().t())
            E[n, h] = d * 2.0 ** -24 * sabs.max(-1).values + 2.0 ** -20
            P = torch.softmax(alpha * (qq @ kk.t()), -1)
            V1[n, h] = P @ vv.abs()
            if dA is not None:
                ga = gA[n, h].abs()
                dabs = (ga * aa[n, h].abs()).sum(-1, keepdim=True)
                W = alpha * P * (ga @ vv.abs().t() + dabs)
                G[n, h, :, 0] = W @ kk.abs()
                G[n, h, :, 1] = W.t() @ qq.abs()
                G[n, h, :, 2] = P.t() @ ga
    out = (E.reshape(N * heads, T), merge_heads(V1))
    if dA is None:
        return out
    return out + (G.permute(0, 2, 1, 3, 4).reshape(N, T, 3 * heads * d),)


def fwd_teams(T):
    """teams of the forward kernel (attention.hip attn_fwd_teams): four from 8 key tiles on"""
    return 4 if T // TILE >= 8 else 2


def restatement(qkv, heads, d, dA=None, lse_in=None, a_in=None, teams=None, drop_tile=None, no_c1=False, no_corr=False,
                alpha=None, layout="qkv", image_offset=0, no_D=False, lse_shift=0, swap_dkdv=False, drop_team1=False):
    """The attention as the kernels walk it, float64.  Forward (dA None): returns a, lse.  Backward: returns dqkv from dA and
    the given lse_in / a_in (what the kernel reads: the saved lse and the forward output), two teams over alternating tiles.
    Mutations: drop_tile (a 64-key tile left out of the forward), no_c1 / no_corr (the merge's or the in-team rescale
    missing), alpha (another scale), layout "kqv" (q and k of a head swapped), image_offset (images n >= 1 read `image_offset`
    channels further on: one head = 3d), no_D (dS without -D_q), lse_shift (P from the lse of query q + shift), swap_dkdv,
    drop_team1 (the backward's team-1 sums lost)."""
    N, T, C3 = qkv.shape
    C = heads * d
    al = 1.0 / math.sqrt(d) if alpha is None else alpha
    x = qkv.double()
    if image_offset:
        flat = torch.cat([x.reshape(-1), torch.zeros(image_offset, dtype=torch.float64)])
        rows = [flat[n * T * C3 + (image_offset if n else 0):][:T * C3].reshape(T, C3) for n in range(N)]
        x = torch.stack(rows)
    q, k, v = split_heads(x, heads, d, layout)
    ntile = T // TILE
    sl = lambda t, i: t[i * TILE:(i + 1) * TILE]
    if dA is None:
        TM = teams or fwd_teams(T)
        a = torch.empty(N, heads, T, d, dtype=torch.float64)
        lse = torch.empty(N, heads, T, dtype=torch.float64)
        for n in range(N):
            for h in range(heads):
                qq, kk, vv = q[n, h], k[n, h], v[n, h]
                states = []
                for team in range(TM):
                    m = torch.full((T,), -1e30, dtype=torch.float64)
                    l = torch.zeros(T, dtype=torch.float64)
                    o = torch.zeros(T, d, dtype=torch.float64)
                    for t in range(team, ntile, TM):
                        if t == drop_tile:
                            continue
                        s = al * (qq @ sl(kk, t).t())
                        mn = torch.maximum(m, s.max(-1).values)
                        corr = torch.ones_like(m) if no_corr else torch.exp(m - mn)
                        p = torch.exp(s - mn[:, None])
                        l = l * corr + p.sum(-1)
                        o = o * corr[:, None] + p @ sl(vv, t)
                        m = mn
                    states.append((m, l, o))
                m, l, o = states[0]
                for m1, l1, o1 in states[1:]:
                    mn = torch.maximum(m, m1)
                    c0 = torch.exp(m - mn)
                    c1 = torch.ones_like(m) if no_c1 else torch.exp(m1 - mn)
                    l = l * c0 + l1 * c1
                    o = o * c0[:, None] + o1 * c1[:, None]
                    m = mn
                a[n, h] = o / l[:, None]
                lse[n, h] = m + torch.log(l)
        return merge_heads(a), lse.reshape(N * heads, T)
    TM = 2 if ntile > 1 else 1
    gA = dA.double().reshape(N, T, heads, d).permute(0, 2, 1, 3)
    aa = a_in.double().reshape(N, T, heads, d).permute(0, 2, 1, 3)
    L = lse_in.double().reshape(N, heads, T)
    g = torch.zeros(N, heads, T, 3, d, dtype=torch.float64)
    for n in range(N):
        for h in range(heads):
            qq, kk, vv, ga = q[n, h], k[n, h], v[n, h], gA[n, h]
            Dq = torch.zeros(T, dtype=torch.float64) if no_D else (ga * aa[n, h]).sum(-1)
            lq = torch.roll(L[n, h], -lse_shift) if lse_shift else L[n, h]

            def ds_p(qi, ki):        # dS and P of query tile qi against key tile ki
                P = torch.exp(al * (sl(qq, qi) @ sl(kk, ki).t()) - sl(lq, qi)[:, None])
                dP = sl(ga, qi) @ sl(vv, ki).t()
                return al * P * (dP - sl(Dq, qi)[:, None]), P

            for i in range(ntile):
                part_q = [torch.zeros(TILE, d, dtype=torch.float64) for _ in range(TM)]
                part_k = [torch.zeros(TILE, d, dtype=torch.float64) for _ in range(TM)]
                part_v = [torch.zeros(TILE, d, dtype=torch.float64) for _ in range(TM)]
                for team in range(TM):
                    for t in range(team, ntile, TM):
                        dS, _ = ds_p(i, t)                   # dQ workgroup of query tile i: key tiles t
                        part_q[team] += dS @ sl(kk, t)
                        dS, P = ds_p(t, i)                   # dK/dV workgroup of key tile i: query tiles t
                        part_k[team] += dS.t() @ sl(qq, t)
                        part_v[team] += P.t() @ sl(ga, t)
                keep = 1 if drop_team1 else TM
                dk, dv = sum(part_k[:keep]), sum(part_v[:keep])
                if swap_dkdv:
                    dk, dv = dv, dk
                g[n, h, i * TILE:(i + 1) * TILE, 0] = sum(part_q[:keep])
                g[n, h, i * TILE:(i + 1) * TILE, 1] = dk
                g[n, h, i * TILE:(i + 1) * TILE, 2] = dv
    return g.permute(0, 2, 1, 3, 4).reshape(N, T, 3 * C)
