"""Which launch every GroupNorm pass gets: the route (csrc/norm.hip gn_route), and for the group-local kernels the part count,
vector width, thread count, grid, LDS bytes and kernel instance that csrc/norm_local.hip plans (gn_local_plan), read on the CPU
through ishap_group_norm32_plan.  The expected values are what the dispatch chose before it was gathered into the planner
(pick_parts / pick_vec / pick_threads, the two launchers' own smem and grid lines and their macro ladders, local_gn / local_gn_bwd,
the full-map launchers' block arithmetic), evaluated for these shapes -- not values read back from the planner.  Without a GPU the
compute-unit count that bounds the part count is the 256 of a whole MI355X.

The cases are the GroupNorm sites of the full model (128^2 input, 256 channels x (1, 1, 2, 3, 4)) on its 32^2, 16^2 and 8^2
levels -- in_layers (SiLU), out_layers (FiLM + SiLU), the attention block's (no SiLU), the downsampling block's pooled form, a
decoder block's skip concatenation, and the backward pass of each with the gradient at the same (GB_SAME), half (GB_UNPOOL) and
twice (GB_SUM4) the resolution, dense and pending -- plus a 64^2 map, no rendezvous record, and batches 2 and 8."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: ((N, H, W, C, backward, pending, film, act, pool, gmode, route),
#        (route taken, parts, VEC, threads, grid x, grid y, LDS bytes, xcd dealing, kernel))
CASES = {
    '32^2 x 256: in_layers GN + SiLU, dense': ((1, 32, 32, 256, 0, 0, 0, 1, 0, 0, 0), (3, 8, 2, 512, 256, 1, 2560, 1, 'gn_local_kernel<2, false, true, false>')),
    '32^2 x 256: in_layers GN + SiLU, pending': ((1, 32, 32, 256, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 512, 256, 1, 2560, 1, 'gn_local_kernel<2, false, true, false>')),
    '32^2 x 256: backward of in_layers, dense gradient': ((1, 32, 32, 256, 1, 0, 0, 1, 0, 0, 0), (3, 8, 2, 512, 256, 1, 2560, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '32^2 x 256: backward of in_layers, pending gradient': ((1, 32, 32, 256, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 512, 256, 1, 2560, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '32^2 x 512: in_layers GN + SiLU, dense': ((1, 32, 32, 512, 0, 0, 0, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_local_kernel<2, false, true, false>')),
    '32^2 x 512: in_layers GN + SiLU, pending': ((1, 32, 32, 512, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_local_kernel<2, false, true, false>')),
    '32^2 x 512: backward of in_layers, dense gradient': ((1, 32, 32, 512, 1, 0, 0, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '32^2 x 512: backward of in_layers, pending gradient': ((1, 32, 32, 512, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '32^2 x 256: out_layers GN + FiLM + SiLU, pending': ((1, 32, 32, 256, 0, 1, 1, 1, 0, 0, 0), (3, 8, 2, 512, 256, 1, 2560, 1, 'gn_local_kernel<2, true, true, false>')),
    '32^2 x 256: backward of out_layers, pending gradient': ((1, 32, 32, 256, 1, 1, 1, 1, 0, 0, 0), (3, 8, 2, 512, 256, 1, 2560, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '32^2 x 512: out_layers GN + FiLM + SiLU, pending': ((1, 32, 32, 512, 0, 1, 1, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_local_kernel<2, true, true, false>')),
    '32^2 x 512: backward of out_layers, pending gradient': ((1, 32, 32, 512, 1, 1, 1, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '32^2 x 512: out_layers GN + FiLM + SiLU, dense': ((1, 32, 32, 512, 0, 0, 1, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_local_kernel<2, true, true, false>')),
    '32^2 x 512: backward of out_layers, dense gradient': ((1, 32, 32, 512, 1, 0, 1, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '32^2 x 512: attention GN (no SiLU), pending': ((1, 32, 32, 512, 0, 1, 0, 0, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_local_kernel<2, false, false, false>')),
    '32^2 x 512: backward of attention GN, pending gradient': ((1, 32, 32, 512, 1, 1, 0, 0, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_bwd_local_kernel<2, false, false, false>')),
    '32^2 x 1280: skip concatenation GN + SiLU, first half pending': ((1, 32, 32, 1280, 0, 1, 0, 1, 0, 0, 0), (3, 8, 4, 1024, 256, 1, 10752, 1, 'gn_local_kernel<4, false, true, false>')),
    "32^2 x 1280: backward of a skip concatenation's GN, pending gradient": ((1, 32, 32, 1280, 1, 1, 0, 1, 0, 0, 0), (3, 8, 4, 1024, 256, 1, 10752, 1, 'gn_bwd_local_kernel<4, false, true, false>')),
    '32^2 x 1024: skip concatenation GN + SiLU, first half pending': ((1, 32, 32, 1024, 0, 1, 0, 1, 0, 0, 0), (3, 8, 4, 1024, 256, 1, 8704, 1, 'gn_local_kernel<4, false, true, false>')),
    "32^2 x 1024: backward of a skip concatenation's GN, pending gradient": ((1, 32, 32, 1024, 1, 1, 0, 1, 0, 0, 0), (3, 8, 4, 1024, 256, 1, 8704, 1, 'gn_bwd_local_kernel<4, false, true, false>')),
    '32^2 x 768: skip concatenation GN + SiLU, first half pending': ((1, 32, 32, 768, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 6656, 1, 'gn_local_kernel<2, false, true, false>')),
    "32^2 x 768: backward of a skip concatenation's GN, pending gradient": ((1, 32, 32, 768, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 1024, 256, 1, 6656, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '32^2 x 512: downsampling in_layers GN + SiLU + pool, dense': ((1, 32, 32, 512, 0, 0, 0, 1, 1, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_local_kernel<2, false, true, true>')),
    '32^2 x 512: downsampling in_layers GN + SiLU + pool, pending': ((1, 32, 32, 512, 0, 1, 0, 1, 1, 0, 0), (3, 8, 2, 1024, 256, 1, 4608, 1, 'gn_local_kernel<2, false, true, true>')),
    '32^2 x 512: backward of the pooled in_layers (GB_UNPOOL), pending gradient': ((1, 32, 32, 512, 1, 1, 0, 1, 0, 1, 0), (3, 8, 2, 1024, 256, 1, 8704, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '32^2 x 512: backward of the pooled in_layers (GB_UNPOOL), dense gradient': ((1, 32, 32, 512, 1, 0, 0, 1, 0, 1, 0), (3, 8, 2, 1024, 256, 1, 8704, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '32^2 x 512: backward of the upsampling in_layers (GB_SUM4), dense gradient': ((1, 32, 32, 512, 1, 0, 0, 1, 0, 2, 0), (3, 8, 2, 1024, 256, 1, 8704, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '32^2 x 512: backward of the upsampling in_layers (GB_SUM4), pending gradient': ((1, 32, 32, 512, 1, 1, 0, 1, 0, 2, 0), (3, 8, 2, 1024, 256, 1, 8704, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '16^2 x 512: in_layers GN + SiLU, dense': ((1, 16, 16, 512, 0, 0, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_local_kernel<2, false, true, false>')),
    '16^2 x 512: in_layers GN + SiLU, pending': ((1, 16, 16, 512, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_local_kernel<2, false, true, false>')),
    '16^2 x 512: backward of in_layers, dense gradient': ((1, 16, 16, 512, 1, 0, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '16^2 x 512: backward of in_layers, pending gradient': ((1, 16, 16, 512, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '16^2 x 768: in_layers GN + SiLU, dense': ((1, 16, 16, 768, 0, 0, 0, 1, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_local_kernel<2, false, true, false>')),
    '16^2 x 768: in_layers GN + SiLU, pending': ((1, 16, 16, 768, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_local_kernel<2, false, true, false>')),
    '16^2 x 768: backward of in_layers, dense gradient': ((1, 16, 16, 768, 1, 0, 0, 1, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '16^2 x 768: backward of in_layers, pending gradient': ((1, 16, 16, 768, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '16^2 x 512: out_layers GN + FiLM + SiLU, pending': ((1, 16, 16, 512, 0, 1, 1, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_local_kernel<2, true, true, false>')),
    '16^2 x 512: backward of out_layers, pending gradient': ((1, 16, 16, 512, 1, 1, 1, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '16^2 x 768: out_layers GN + FiLM + SiLU, pending': ((1, 16, 16, 768, 0, 1, 1, 1, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_local_kernel<2, true, true, false>')),
    '16^2 x 768: backward of out_layers, pending gradient': ((1, 16, 16, 768, 1, 1, 1, 1, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '16^2 x 1024: out_layers GN + FiLM + SiLU, pending': ((1, 16, 16, 1024, 0, 1, 1, 1, 0, 0, 0), (3, 8, 2, 512, 256, 1, 2560, 1, 'gn_local_kernel<2, true, true, false>')),
    '16^2 x 1024: backward of out_layers, pending gradient': ((1, 16, 16, 1024, 1, 1, 1, 1, 0, 0, 0), (3, 8, 2, 512, 256, 1, 2560, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '16^2 x 768: out_layers GN + FiLM + SiLU, dense': ((1, 16, 16, 768, 0, 0, 1, 1, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_local_kernel<2, true, true, false>')),
    '16^2 x 768: backward of out_layers, dense gradient': ((1, 16, 16, 768, 1, 0, 1, 1, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '16^2 x 768: attention GN (no SiLU), pending': ((1, 16, 16, 768, 0, 1, 0, 0, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_local_kernel<2, false, false, false>')),
    '16^2 x 768: backward of attention GN, pending gradient': ((1, 16, 16, 768, 1, 1, 0, 0, 0, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_bwd_local_kernel<2, false, false, false>')),
    '16^2 x 1792: skip concatenation GN + SiLU, first half pending': ((1, 16, 16, 1792, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 896, 256, 1, 4096, 1, 'gn_local_kernel<2, false, true, false>')),
    "16^2 x 1792: backward of a skip concatenation's GN, pending gradient": ((1, 16, 16, 1792, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 896, 256, 1, 4096, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '16^2 x 1536: skip concatenation GN + SiLU, first half pending': ((1, 16, 16, 1536, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 768, 256, 1, 3584, 1, 'gn_local_kernel<2, false, true, false>')),
    "16^2 x 1536: backward of a skip concatenation's GN, pending gradient": ((1, 16, 16, 1536, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 768, 256, 1, 3584, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '16^2 x 1280: skip concatenation GN + SiLU, first half pending': ((1, 16, 16, 1280, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 640, 256, 1, 3072, 1, 'gn_local_kernel<2, false, true, false>')),
    "16^2 x 1280: backward of a skip concatenation's GN, pending gradient": ((1, 16, 16, 1280, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 640, 256, 1, 3072, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '16^2 x 768: downsampling in_layers GN + SiLU + pool, dense': ((1, 16, 16, 768, 0, 0, 0, 1, 1, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_local_kernel<2, false, true, true>')),
    '16^2 x 768: downsampling in_layers GN + SiLU + pool, pending': ((1, 16, 16, 768, 0, 1, 0, 1, 1, 0, 0), (3, 8, 2, 384, 256, 1, 2048, 1, 'gn_local_kernel<2, false, true, true>')),
    '16^2 x 768: backward of the pooled in_layers (GB_UNPOOL), pending gradient': ((1, 16, 16, 768, 1, 1, 0, 1, 0, 1, 0), (3, 8, 2, 384, 256, 1, 3584, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '16^2 x 768: backward of the pooled in_layers (GB_UNPOOL), dense gradient': ((1, 16, 16, 768, 1, 0, 0, 1, 0, 1, 0), (3, 8, 2, 384, 256, 1, 3584, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '16^2 x 768: backward of the upsampling in_layers (GB_SUM4), dense gradient': ((1, 16, 16, 768, 1, 0, 0, 1, 0, 2, 0), (3, 8, 2, 384, 256, 1, 3584, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '16^2 x 768: backward of the upsampling in_layers (GB_SUM4), pending gradient': ((1, 16, 16, 768, 1, 1, 0, 1, 0, 2, 0), (3, 8, 2, 384, 256, 1, 3584, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '8^2 x 768: in_layers GN + SiLU, dense': ((1, 8, 8, 768, 0, 0, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 896, 1, 'gn_local_kernel<2, false, true, false>')),
    '8^2 x 768: in_layers GN + SiLU, pending': ((1, 8, 8, 768, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 896, 1, 'gn_local_kernel<2, false, true, false>')),
    '8^2 x 768: backward of in_layers, dense gradient': ((1, 8, 8, 768, 1, 0, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 896, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '8^2 x 768: backward of in_layers, pending gradient': ((1, 8, 8, 768, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 896, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '8^2 x 1024: in_layers GN + SiLU, dense': ((1, 8, 8, 1024, 0, 0, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_local_kernel<2, false, true, false>')),
    '8^2 x 1024: in_layers GN + SiLU, pending': ((1, 8, 8, 1024, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_local_kernel<2, false, true, false>')),
    '8^2 x 1024: backward of in_layers, dense gradient': ((1, 8, 8, 1024, 1, 0, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '8^2 x 1024: backward of in_layers, pending gradient': ((1, 8, 8, 1024, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '8^2 x 768: out_layers GN + FiLM + SiLU, pending': ((1, 8, 8, 768, 0, 1, 1, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 896, 1, 'gn_local_kernel<2, true, true, false>')),
    '8^2 x 768: backward of out_layers, pending gradient': ((1, 8, 8, 768, 1, 1, 1, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 896, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '8^2 x 1024: out_layers GN + FiLM + SiLU, pending': ((1, 8, 8, 1024, 0, 1, 1, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_local_kernel<2, true, true, false>')),
    '8^2 x 1024: backward of out_layers, pending gradient': ((1, 8, 8, 1024, 1, 1, 1, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '8^2 x 1024: out_layers GN + FiLM + SiLU, dense': ((1, 8, 8, 1024, 0, 0, 1, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_local_kernel<2, true, true, false>')),
    '8^2 x 1024: backward of out_layers, dense gradient': ((1, 8, 8, 1024, 1, 0, 1, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_bwd_local_kernel<2, true, true, false>')),
    '8^2 x 1024: attention GN (no SiLU), pending': ((1, 8, 8, 1024, 0, 1, 0, 0, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_local_kernel<2, false, false, false>')),
    '8^2 x 1024: backward of attention GN, pending gradient': ((1, 8, 8, 1024, 1, 1, 0, 0, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_bwd_local_kernel<2, false, false, false>')),
    '8^2 x 2048: skip concatenation GN + SiLU, first half pending': ((1, 8, 8, 2048, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_local_kernel<2, false, true, false>')),
    "8^2 x 2048: backward of a skip concatenation's GN, pending gradient": ((1, 8, 8, 2048, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '8^2 x 1792: skip concatenation GN + SiLU, first half pending': ((1, 8, 8, 1792, 0, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1408, 1, 'gn_local_kernel<2, false, true, false>')),
    "8^2 x 1792: backward of a skip concatenation's GN, pending gradient": ((1, 8, 8, 1792, 1, 1, 0, 1, 0, 0, 0), (3, 8, 2, 256, 256, 1, 1408, 1, 'gn_bwd_local_kernel<2, false, true, false>')),
    '8^2 x 1024: backward of the upsampling in_layers (GB_SUM4), dense gradient': ((1, 8, 8, 1024, 1, 0, 0, 1, 0, 2, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '8^2 x 1024: backward of the upsampling in_layers (GB_SUM4), pending gradient': ((1, 8, 8, 1024, 1, 1, 0, 1, 0, 2, 0), (3, 8, 2, 256, 256, 1, 1536, 1, 'gn_bwd_local_kernel<2, false, true, true>')),
    '64^2 x 256: forward takes the epilogue-sum route': ((1, 64, 64, 256, 0, 0, 0, 1, 0, 0, 0), (4, 0, 8, 256, 512, 1, 0, 0, 'gn_apply_kernel<false, true, false, false>')),
    '64^2 x 256: backward takes the two-pass route': ((1, 64, 64, 256, 1, 0, 0, 1, 0, 0, 0), (1, 0, 8, 256, 512, 1, 0, 0, 'gn_bwd_apply_kernel<false, true>')),
    '64^2 x 512: FiLM forward on the full map': ((1, 64, 64, 512, 0, 0, 1, 1, 0, 0, 0), (4, 0, 8, 256, 1024, 1, 0, 0, 'gn_apply_kernel<true, true, false, false>')),
    '64^2 x 256: pooled forward on the full map': ((1, 64, 64, 256, 0, 0, 0, 1, 1, 0, 0), (4, 0, 8, 256, 128, 1, 0, 0, 'gn_apply_kernel<false, true, true, false>')),
    '8^2 x 1024 without a record: one workgroup per group': ((1, 8, 8, 1024, 0, 0, 0, 1, 0, 0, 2), (2, 1, 2, 1024, 32, 1, 4608, 0, 'gn_local_kernel<2, false, true, false>')),
    '32^2 x 512 backward without a record': ((1, 32, 32, 512, 1, 0, 0, 1, 0, 0, 2), (2, 1, 8, 1024, 32, 1, 33280, 0, 'gn_bwd_local_kernel<8, false, true, false>')),
    'batch 8, 32^2 x 512: the 256-CU bound leaves one part': ((8, 32, 32, 512, 0, 0, 0, 1, 0, 0, 0), (3, 1, 8, 1024, 32, 8, 33280, 0, 'gn_local_kernel<8, false, true, false>')),
    'batch 8, 8^2 x 1024 backward: one part': ((8, 8, 8, 1024, 1, 1, 0, 1, 0, 0, 0), (3, 1, 2, 1024, 32, 8, 4608, 0, 'gn_bwd_local_kernel<2, false, true, false>')),
    'batch 2, 16^2 x 768: four parts': ((2, 16, 16, 768, 0, 0, 0, 1, 0, 0, 0), (3, 4, 2, 768, 128, 2, 3584, 1, 'gn_local_kernel<2, false, true, false>')),
    '8^2 x 1024 dense forward with a record (worked by hand)': ((1, 8, 8, 1024, 0, 0, 0, 1, 0, 0, 3), (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_local_kernel<2, false, true, false>')),
}

# switch -> some cases it changes (or must leave alone), with their plan under it
SWITCHES = {
    "ISHAP_GN_PARTS=1": {          # one workgroup per (image, group): wider vectors, more LDS per workgroup; the full maps untouched
        '8^2 x 1024 dense forward with a record (worked by hand)': (3, 1, 2, 1024, 32, 1, 4608, 0, 'gn_local_kernel<2, false, true, false>'),
        '32^2 x 512: in_layers GN + SiLU, pending': (3, 1, 4, 1024, 32, 1, 33280, 0, 'gn_local_kernel<4, false, true, false>'),
        '16^2 x 768: backward of the pooled in_layers (GB_UNPOOL), pending gradient': (3, 1, 4, 1024, 32, 1, 25088, 0, 'gn_bwd_local_kernel<4, false, true, true>'),
        '64^2 x 256: forward takes the epilogue-sum route': (4, 0, 8, 256, 512, 1, 0, 0, 'gn_apply_kernel<false, true, false, false>'),
    },
    "ISHAP_GN_XCD=0": {            # the same launches, parts dealt to consecutive workgroups
        '8^2 x 1024 dense forward with a record (worked by hand)': (3, 8, 2, 256, 256, 1, 1024, 0, 'gn_local_kernel<2, false, true, false>'),
        '16^2 x 768: backward of in_layers, pending gradient': (3, 8, 2, 384, 256, 1, 2048, 0, 'gn_bwd_local_kernel<2, false, true, false>'),
        'batch 8, 32^2 x 512: the 256-CU bound leaves one part': (3, 1, 8, 1024, 32, 8, 33280, 0, 'gn_local_kernel<8, false, true, false>'),
    },
    "ISHAP_LOCAL_GN=0": {          # route 0 leaves the small maps to the full-map kernels; an explicit route 2 stays group-local
        '8^2 x 1024 dense forward with a record (worked by hand)': (3, 8, 2, 256, 256, 1, 1024, 1, 'gn_local_kernel<2, false, true, false>'),
        '32^2 x 512: downsampling in_layers GN + SiLU + pool, pending': (4, 0, 8, 256, 64, 1, 0, 0, 'gn_apply_kernel<false, true, true, false>'),
        '16^2 x 768: out_layers GN + FiLM + SiLU, pending': (4, 0, 8, 256, 96, 1, 0, 0, 'gn_apply_kernel<true, true, false, false>'),
        '8^2 x 1024: backward of the upsampling in_layers (GB_SUM4), dense gradient': (1, 0, 8, 256, 32, 1, 0, 0, 'gn_bwd_apply_kernel<false, true>'),
        '8^2 x 1024 without a record: one workgroup per group': (2, 1, 2, 1024, 32, 1, 4608, 0, 'gn_local_kernel<2, false, true, false>'),
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
    o = [C.c_int() for _ in range(8)]
    kern = C.create_string_buffer(96)
    rc = L.ishap_group_norm32_plan(*args, *[C.byref(v) for v in o], kern, len(kern))
    out[name] = [v.value for v in o] + [kern.value.decode()] if rc == 0 else rc
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


def test_every_site_gets_the_launch_it_got_before(plans):
    got = plans[""]
    bad = {n: (got[n], exp) for n, (_, exp) in CASES.items() if got[n] != exp}
    assert not bad, bad
    kernels = {exp[8] for _, exp in CASES.values()}
    for form in ("gn_local_kernel<8,", "gn_local_kernel<4,", "gn_local_kernel<2,", "gn_bwd_local_kernel<4,", "gn_bwd_local_kernel<2,",
                 "true>", "gn_apply_kernel<", "gn_bwd_apply_kernel<"):
        assert any(form in k for k in kernels), form


def test_the_case_worked_by_hand():
    """N = 1, 8x8, C = 1024, dense, forward, record present.  cpg = 32, H*W = 64.  pick_parts doubles while 64 / parts * 32 >= 128
    elements and 32 * parts <= 256 workgroups: 8 parts of 8 pixels.  pick_vec(32, 8, dense): 8 and 4 leave 32 and 64 units, fewer
    than 1024, so it ends at 2; 8 * 16 = 128 units -> 256 threads.  LDS: 512 bytes of scratch + 8 * 32 fp16 values."""
    exp = CASES["8^2 x 1024 dense forward with a record (worked by hand)"][1]
    assert exp == (3, 8, 2, 256, 256, 1, 512 + 8 * 32 * 2, 1, "gn_local_kernel<2, false, true, false>")


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_each_switch_changes_what_it_documents(plans, switch):
    got = plans[switch]
    bad = {n: (got[n], want) for n, want in SWITCHES[switch].items() if got[n] != want}
    assert not bad, bad


def test_plan_reports_bad_arguments():
    from ishapediting_amd import _lib
    L = _lib.lib()
    none = [None] * 8
    kern = C.create_string_buffer(8)
    assert L.ishap_group_norm32_plan(1, 8, 8, 1024, 0, 0, 0, 1, 0, 0, 0, *none, kern, len(kern)) == -2        # short name buffer
    assert L.ishap_group_norm32_plan(1, 8, 8, 1000, 0, 0, 0, 1, 0, 0, 0, *none, None, 0) == -2                # C % 32
    assert L.ishap_group_norm32_plan(1, 8, 8, 1024, 1, 0, 0, 1, 0, 0, 4, *none, None, 0) == -2                # no backward route 4
    assert L.ishap_group_norm32_plan(1, 64, 64, 1024, 0, 0, 0, 1, 0, 0, 2, *none, None, 0) == -2              # does not fit in LDS
