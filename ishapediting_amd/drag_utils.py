"""Drop-in mirror of the reference's drag_utils.py call surface (DragStuff, synthesize_latent,
resize_feat_align, make_offsets, get_args) with the arithmetic on libishap_hip.so.

What differs from the reference by design (all inside the boundary, results equal within tolerance):
  * the guidance-feature cache stays on the device as the raw fp16 NHWC taps (reference: 170 resized fp32
    copies on the host, 1.42 GB, re-uploaded every step -- drag_utils.py:276,352);
  * the drag loss and its gradient w.r.t. the tap come from hand-written kernels and the UNet input
    gradient from a hand-written backward that computes no weight gradients (reference: autograd,
    drag_utils.py:383, which also computes and discards every weight gradient);
  * lattice / mask setup runs on the device (reference: Python sets of tuples, drag_utils.py:325-334);
  * the dense decode keeps the 256^3 volume on the device (reference: 336 chunked host round trips).
"""
from __future__ import annotations

import argparse
import collections
import copy
import ctypes as C
import os
from argparse import Namespace
from typing import List, Optional

import numpy as np
import torch as th

from . import _lib
from .script_util import args_to_dict, create_model_and_diffusion, model_and_diffusion_defaults
from .triplane_decoder import MultiTriplane, decode_planes_grid, decode_volume, prepare_planes
from . import mesh as mesh_backend
from .volume import clean_volume


def get_args(argv=None):
    """drag_utils.py:23-58.  The reference parses sys.argv at class-definition time (:176); here the parser
    only sees `argv` (default: no arguments) so importing this module never consumes the host program's flags."""
    parser = argparse.ArgumentParser(description="Generate a set of triplane and their corresponding meshes")
    parser.add_argument("--resolution", type=str, default=128, required=False)
    parser.add_argument("--num_steps", type=int, default=200, required=False)
    parser.add_argument("--shape_resolution", type=int, default=256, required=False)
    parser.add_argument("--w_time", type=int, default=170, required=False)
    parser.add_argument("--feat_layer", type=int, default=8, required=False)
    parser.add_argument("--loss_type", type=str, default="l2")
    parser.add_argument("--points_size", type=int, default=200000)
    parser.add_argument("--points_uniform_ratio", type=float, default=0.5)
    args = parser.parse_args([] if argv is None else argv)
    return Namespace(
        clip_denoised=True, num_samples=1, batch_size=1, use_ddim=False, model_path=None, stats_dir=None,
        num_steps=args.num_steps, explicit_normalization=True, save_dir=None, save_intermediate=False,
        save_timestep_interval=20, image_size=int(args.resolution), num_channels=256, num_res_blocks=2, num_heads=4,
        num_heads_upsample=-1, num_head_channels=64, attention_resolutions="32,16,8", channel_mult="", dropout=0.1,
        class_cond=False, shape_resolution=args.shape_resolution, use_checkpoint=False, use_scale_shift_norm=True,
        resblock_updown=True, use_fp16=True, use_new_attention_order=False, in_out_channels=96, learn_sigma=True,
        diffusion_steps=1000, noise_schedule="linear", timestep_respacing=str(args.num_steps), w_time=args.w_time,
        feat_layer=args.feat_layer, points_size=args.points_size, points_uniform_ratio=args.points_uniform_ratio,
        loss_type=args.loss_type, use_kl=False, predict_xstart=False, rescale_timesteps=False, decoder_ckpt=None,
        rescale_learned_sigmas=False)


def make_offsets(r, device):
    """drag_utils.py:134-138."""
    p = th.arange(-r, r + 1, device=device)
    px, py, pz = th.meshgrid(p, p, p, indexing="ij")
    return th.stack([px.reshape(-1), py.reshape(-1), pz.reshape(-1)], dim=-1)


def _nearest_channel_index(c: int, e: int) -> np.ndarray:
    """Source indices of F.interpolate(..., size=e) 'nearest' over an axis of length c (drag_utils.py:146-151)."""
    return np.minimum(np.floor(np.arange(e, dtype=np.float32) * np.float32(c / e)).astype(np.int64), c - 1)


def feat_channel_map(channels: int) -> np.ndarray:
    """(plane, c) -> tap channel, i.e. resize_feat_align as an index table: int32 [3][2*(half//3)]."""
    assert channels % 2 == 0
    half = channels // 2
    e = half - half % 3
    idx = _nearest_channel_index(half, e) if half % 3 else np.arange(half)
    per = e // 3
    out = np.zeros((3, 2 * per), dtype=np.int32)
    for p in range(3):
        out[p, :per] = idx[p * per:(p + 1) * per]
        out[p, per:] = half + idx[p * per:(p + 1) * per]
    return out


def resize_feat_align(feature, cat_var=True):
    """drag_utils.py:141-159 (index gather; layout work only)."""
    batch_num, channel_num = feature.shape[:2]
    assert not channel_num % 2 and batch_num == 1
    cm = th.as_tensor(feat_channel_map(channel_num), device=feature.device, dtype=th.long)
    per = cm.shape[1] // 2
    if not cat_var:
        cm = cm[:, :per]
    return feature[0][cm.reshape(-1)].reshape(3, -1, feature.shape[2], feature.shape[3]).type(th.float32)


_FUSED_UPDATE = os.environ.get("ISHAP_FUSED_UPDATE", "1") == "1"     # guided update inside the DDPM step kernel (0: two launches, for A/B)
_OVERLAP_TAIL = os.environ.get("ISHAP_OVERLAP_TAIL", "1") == "1"      # round 5: on by default (see training())
# training() runs the forward of its first guided step once per loaded shape and puts its kept state back in later edits (0: every
# edit runs all its forwards)
_FIRST_STEP_REUSE = os.environ.get("ISHAP_FIRST_STEP_REUSE", "1") == "1"


def check_weight_map(w, W: int) -> th.Tensor:
    """A [3, W, W] map of finite weights >= 0 (tensor or array) -> a float32 tensor; ValueError otherwise."""
    w = w.detach() if th.is_tensor(w) else th.as_tensor(np.asarray(w))
    if tuple(w.shape) != (3, W, W):
        raise ValueError(f"weights must be a [3, {W}, {W}] map (one [row, col] slice per plane), got {tuple(w.shape)}")
    w = w.to(th.float32)
    if not bool(th.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("weights must be finite and >= 0")
    return w


def check_region_cof(cof: float, has_regions: bool, what: str = "cof"):
    """Regions act on the preservation term only, and with cof <= 0 there is none."""
    if has_regions and not cof > 0:
        raise ValueError(f"{what} = {cof}: keep / free regions and weights scale the preservation term, which needs cof > 0")


def pack_handles(sources, targets):
    """K edits' handle arrays -> the packed form of ishap_drag_batch_args: (sources [H, 3], targets [H, 3] float32 tensors on the
    CPU, CSR offsets list of K + 1 ints; edit e owns rows offsets[e]:offsets[e + 1])."""
    if len(sources) != len(targets):
        raise ValueError(f"{len(sources)} source sets but {len(targets)} target sets: one of each per edit")
    if len(sources) == 0:
        raise ValueError("no edits")
    src, tgt, offs = [], [], [0]
    for e, (s_, t_) in enumerate(zip(sources, targets)):
        s_ = (s_.detach().cpu() if th.is_tensor(s_) else th.as_tensor(np.asarray(s_))).to(th.float32).reshape(-1, 3)
        t_ = (t_.detach().cpu() if th.is_tensor(t_) else th.as_tensor(np.asarray(t_))).to(th.float32).reshape(-1, 3)
        if s_.shape[0] != t_.shape[0] or s_.shape[0] == 0:
            raise ValueError(f"edit {e}: {s_.shape[0]} sources and {t_.shape[0]} targets (need the same, non-zero count)")
        src.append(s_)
        tgt.append(t_)
        offs.append(offs[-1] + s_.shape[0])
    return th.cat(src).contiguous(), th.cat(tgt).contiguous(), offs


def check_edit_count(K: int, max_edits: int):
    if K > max_edits:
        raise ValueError(f"{K} edits requested but this DragStuff was built for max_edits={max_edits}")
    if K < 1:
        raise ValueError("no edits")


def per_edit(value, K: int, name: str) -> List[float]:
    """A float (every edit) or a length-K sequence (one per edit) -> K floats."""
    if th.is_tensor(value):
        value = value.detach().cpu().reshape(-1).tolist() if value.dim() else float(value)
    if isinstance(value, (int, float, np.floating, np.integer)):
        return [float(value)] * K
    vals = [float(v) for v in value]
    if len(vals) != K:
        raise ValueError(f"{name}: {len(vals)} values for {K} edits (give one float or one value per edit)")
    return vals


def per_edit_any(value, K: int, name: str) -> list:
    """One value (every edit) or a list / tuple of K values -> K values."""
    if isinstance(value, (list, tuple)):
        if len(value) != K:
            raise ValueError(f"{name}: {len(value)} values for {K} edits (give one value or one per edit)")
        return list(value)
    return [value] * K


def per_edit_region(value, K: int, name: str) -> list:
    """keep / free / weights of training_batch -> K entries.  None or a single region / map: every edit gets it; a list of K
    entries (each None, a region, a list of regions, or a map): one per edit."""
    if value is None or not isinstance(value, (list, tuple)):
        return [value] * K
    if len(value) != K:
        raise ValueError(f"{name}: {len(value)} entries for {K} edits (give one value or a list with one entry, or None, per edit)")
    return list(value)


class BatchDragKernels:
    """Device state + calls of the drag loss for E edits at once (ishap_drag_batch_*): one scratch buffer, one loss scale.  One
    edit is E = 1 (DragKernels below)."""

    def __init__(self, device, E: int, W: int, ld: int, chmap, r: int, voxel: float, loss_type: str = "l2"):
        self.device = th.device(device)
        self.E, self.W, self.ld, self.r, self.voxel = int(E), W, ld, r, float(voxel)
        self.l1 = 1 if loss_type == "l1" else 0
        self.chmap = th.as_tensor(np.asarray(chmap), dtype=th.int32).reshape(3, -1).contiguous().to(self.device)
        self.Cc = self.chmap.shape[1]
        self.bits = th.zeros(1, dtype=th.int32, device=self.device)
        self.scale2 = th.ones(2, dtype=th.float32, device=self.device)
        self.sources = self.targets = self.weights = None
        self._L = _lib.lib()
        nbytes = int(self._L.ishap_drag_batch_scratch_bytes(self.E, W, ld))
        if nbytes <= 0:
            raise ValueError(f"drag batch: bad dimensions E={E}, W={W}, ld={ld}")
        self.scratch = th.zeros(nbytes, dtype=th.uint8, device=self.device)
        self.grad = th.empty((self.E, W * W, ld), dtype=th.float32, device=self.device)
        self.loss = th.zeros(self.E, dtype=th.float32, device=self.device)
        self.cot = th.empty((self.E, W * W, ld), dtype=th.float16, device=self.device)
        # closed loop (retarget): `targets` stays the final targets; the loss reads the goals at _aim_ptr once a retarget has run
        self.goals = self.remaining = self.arrived = self.done = None
        self._aim_ptr = None
        self._aim_keep = None         # whatever owns the memory at _aim_ptr when that is not self.goals (the loop's table)

    def _call(self, name: str, *args):
        _lib.call(self.device, name, *args)

    def _targets_ptr(self) -> int:
        """What the loss kernels read as targets: the final targets, or the goals of the last retarget."""
        return self.targets.data_ptr() if self._aim_ptr is None else self._aim_ptr

    def _args(self, orig_stride: int = 0) -> _lib.DragBatchArgsC:
        return _lib.DragBatchArgsC(self.E, self.W, self.ld, self.Cc, self.chmap.data_ptr(), self.sources.data_ptr(),
                                   self._targets_ptr(), self._offs, self.r, self.voxel, self._cof, self.l1, int(orig_stride),
                                   self.scratch.data_ptr(), self.scratch.numel(), _lib.ptr(self.weights), 3 * self.W * self.W)

    def setup(self, sources, targets, cof, weights=None):
        """sources / targets: lists of E handle arrays; cof: a float or E floats; weights: None, or a list of E entries, each None
        or a [3, W, W] map (regions.plane_weights) for an edit with cof > 0.  All None selects the unweighted launch; otherwise
        an edit without a map reads a map of ones, which gives bitwise its unweighted result."""
        src, tgt, offs = pack_handles(sources, targets)
        if len(offs) - 1 != self.E:
            raise ValueError(f"{len(offs) - 1} edits given to drag kernels set up for {self.E}")
        self._setup(src.to(self.device), tgt.to(self.device), offs, cof, weights)

    def _setup(self, src, tgt, offs, cof, weights):
        """setup() on packed handles: src / tgt float32 [H, 3] on the device, offs the E + 1 CSR offsets."""
        cofs = per_edit(cof, self.E, "cof")
        self.weights = None
        if weights is not None:
            weights = list(weights)
            if len(weights) != self.E:
                raise ValueError(f"weights: {len(weights)} entries for {self.E} edits (give one map or None per edit)")
            for e, w in enumerate(weights):
                check_region_cof(cofs[e], w is not None, f"cof[{e}]")
            maps = [None if w is None else check_weight_map(w, self.W).to(device=self.device).contiguous() for w in weights]
            if self.E == 1 and maps[0] is not None:
                self.weights = maps[0][None]          # one edit reads its map where it is
            elif any(m is not None for m in maps):
                self.weights = th.ones((self.E, 3, self.W, self.W), dtype=th.float32, device=self.device)
                for e, m in enumerate(maps):
                    if m is not None:
                        self.weights[e].copy_(m)
        self.sources, self.targets = src, tgt
        self.offsets = list(offs)
        self._offs = (C.c_int * (self.E + 1))(*offs)
        self.cof = cofs
        self._cof = (C.c_float * self.E)(*self.cof)
        self.goals = self.remaining = self.arrived = self.done = None
        self._aim_ptr = self._aim_keep = None
        self._call("ishap_drag_batch_setup", C.byref(self._args()))

    def retarget(self, K, step, arrive):
        """Re-aim the loss (ishap_drag_batch_retarget) after setup(): K int [H, 3], each handle's tracked voxel
        offset from its source; step > 0 (may be inf), the lead in voxels; arrive >= 0 (each a float, or one value per edit).
        Writes the object's goals buffer [H, 3], which every later loss call reads in place of the targets, and rebuilds the
        touched sets and mask counts for it; `targets` stays the final targets.  Returns (goals, remaining [H] float32, arrived [H]
        int32, done [E] int32), device tensors the next call overwrites."""
        if self.sources is None:
            raise RuntimeError("retarget: call setup() first")
        H = self.sources.shape[0]
        K = _lib.tensor(K, th.int32, self.device)
        if tuple(K.shape) != (H, 3):
            raise ValueError(f"retarget: K must be [{H}, 3], got {tuple(K.shape)}")
        if self.goals is None:
            self.goals = th.empty((H, 3), dtype=th.float32, device=self.device)
            self.remaining = th.empty(H, dtype=th.float32, device=self.device)
            self.arrived = th.empty(H, dtype=th.int32, device=self.device)
            self.done = th.empty(self.E, dtype=th.int32, device=self.device)
        self.retarget_raw(K.data_ptr(), self.goals.data_ptr(), self.remaining.data_ptr(), self.arrived.data_ptr(),
                          self.done.data_ptr(), step, arrive)
        return self.goals, self.remaining, self.arrived, self.done

    def retarget_raw(self, k: int, goals: int, remaining: int, arrived: int, done: int, step, arrive):
        """retarget() on device addresses (the guided loop's form: rows of its tables; no tensor is made per step).  The loss
        calls that follow read `goals`."""
        keep, self._aim_ptr = self._aim_ptr, goals
        try:
            if any(not isinstance(v, (int, float, np.floating, np.integer)) for v in (step, arrive)):     # one lead / arrival radius per edit
                st, ar = per_edit(step, self.E, "step"), per_edit(arrive, self.E, "arrive")
                self._call("ishap_drag_batch_retarget_each", C.byref(self._args()), self.targets.data_ptr(), k,
                           (C.c_float * self.E)(*st), (C.c_float * self.E)(*ar), remaining, arrived, done)
            else:
                self._call("ishap_drag_batch_retarget", C.byref(self._args()), self.targets.data_ptr(), k, float(step),
                           float(arrive), remaining, arrived, done)
        except Exception:
            self._aim_ptr = keep          # refused before any launch: the loss keeps reading what it read
            raise

    def scratch_parts(self) -> dict:
        """Views of the scratch buffer as api.hip carves it (every part on a 256-byte boundary): gfx int64 [E, W*W*ld], acc int64
        [E, 2], nmask int32 [E], touched uint8 [E, 3*W*W], chan_weight uint8 [3*ld]."""
        E, W, ld = self.E, self.W, self.ld
        up = lambda v: (v + 255) & ~255      # noqa: E731
        o_acc = up(E * W * W * ld * 8)
        o_nmask = up(o_acc + E * 16)
        o_touched = up(o_nmask + E * 4)
        o_chw = up(o_touched + E * 3 * W * W)
        s = self.scratch
        return {"gfx": s[:E * W * W * ld * 8].view(th.int64).reshape(E, -1), "acc": s[o_acc:o_acc + E * 16].view(th.int64).reshape(E, 2),
                "nmask": s[o_nmask:o_nmask + E * 4].view(th.int32), "touched": s[o_touched:o_touched + E * 3 * W * W].reshape(E, -1),
                "chan_weight": s[o_chw:o_chw + 3 * ld]}

    def loss_grad_ptr(self, edit_ptr: int, orig_ptr: int, orig_stride: int = 0):
        """edit: [E][W*W][ld] fp16; orig: edit e's guidance at orig + e * orig_stride halfs (0: one guidance for all edits)."""
        self._call("ishap_drag_batch_loss_grad", C.byref(self._args(orig_stride)), edit_ptr, orig_ptr, self.grad.data_ptr(),
                   self.loss.data_ptr())
        return self.grad, self.loss

    def loss_grad(self, edit: th.Tensor, orig: th.Tensor):
        """loss_grad_ptr on tensors: edit the E taps, orig E guidance taps or one for all edits."""
        assert edit.dtype == th.float16 and orig.dtype == th.float16 and edit.is_contiguous() and orig.is_contiguous()
        n = self.W * self.W * self.ld
        assert edit.numel() == self.E * n and orig.numel() in (n, self.E * n)
        return self.loss_grad_ptr(edit.data_ptr(), orig.data_ptr(), 0 if orig.numel() == n else n)

    def loss_cotangent_ptr(self, edit_ptr: int, orig_ptr: int, orig_stride: int = 0, loss_out=None):
        """losses + gradients + the batch's fp16 cotangent (one loss scale, scale2) in three launches; `loss_out`: device float[E]."""
        loss = self.loss if loss_out is None else loss_out
        self._call("ishap_drag_batch_loss_cotangent", C.byref(self._args(orig_stride)), edit_ptr, orig_ptr,
                   self.grad.data_ptr(), loss.data_ptr(), self.cot.data_ptr(), self.bits.data_ptr(), self.scale2.data_ptr())
        return self.cot, self.scale2

    def scaled_cotangent(self):
        """fp32 gradient -> fp16 cotangent * 2^k (k from max|g|) so the fp16 backward neither under- nor overflows."""
        self._call("ishap_grad_to_scaled_f16", self.grad.data_ptr(), self.cot.data_ptr(), self.bits.data_ptr(),
                   self.scale2.data_ptr(), self.grad.numel())
        return self.cot, self.scale2


class DragKernels(BatchDragKernels):
    """One edit (drag_utils.py:309-334 setup, :355-383 per step): BatchDragKernels with E = 1, set up from one handle array, one
    cof and one map, its buffers seen without the edit axis (the same memory)."""

    def __init__(self, device, W: int, ld: int, chmap, r: int, voxel: float, loss_type: str = "l2"):
        super().__init__(device, 1, W, ld, chmap, r, voxel, loss_type)
        self.grad, self.cot = self.grad[0], self.cot[0]
        part = self.scratch_parts()
        self.touched, self.gfx, self.acc = part["touched"][0], part["gfx"][0], part["acc"][0]
        self.nmask, self.chan_weight = part["nmask"], part["chan_weight"]

    def setup(self, sources, targets, cof: float, weights=None):
        """weights: None, or a [3, W, W] map of the preservation term's per-texel weights (regions.plane_weights); needs cof > 0.
        A map selects the weighted gather kernel; a map of ones gives bitwise the results of None.  Handles already on the
        device stay there: one edit needs no packing, so nothing comes back to the host."""
        check_region_cof(float(cof), weights is not None)

        def pts(v):
            v = v.detach() if th.is_tensor(v) else th.as_tensor(np.asarray(v))
            return v.to(device=self.device, dtype=th.float32).reshape(-1, 3).contiguous()
        src, tgt = pts(sources), pts(targets)
        if src.shape[0] != tgt.shape[0] or src.shape[0] == 0:
            raise ValueError(f"{src.shape[0]} sources and {tgt.shape[0]} targets (need the same, non-zero count)")
        self._setup(src, tgt, [0, src.shape[0]], float(cof), None if weights is None else [weights])
        self.weights = None if self.weights is None else self.weights[0]


Track = collections.namedtuple("Track", "offsets positions dist dist0 volume")
TRACK_DEFAULTS = {"radius": 4, "patch": 2, "every": 1}


def track_options(track) -> Optional[dict]:
    """The `track` keyword of training() / training_part() / training_batch(): None or False (off), True (the defaults) or a dict
    with any of radius, patch, every -> None or the full dict."""
    if track is None or track is False:
        return None
    opts = dict(TRACK_DEFAULTS)
    if track is not True:
        unknown = set(track) - set(opts)
        if unknown:
            raise ValueError(f"track: unknown keys {sorted(unknown)} (radius, patch, every)")
        opts.update({k: int(v) for k, v in track.items()})
    if opts["every"] < 1:
        raise ValueError(f"track: every = {opts['every']} (must be >= 1)")
    return opts


class HandleTracker:
    """Where each drag handle went, in feature space (ishap_drag_track): for every handle the offset k in
    [-radius, radius]^3 voxels whose patch of the edited tap is nearest in L1 to the guidance tap's patch at the source.
    Offsets are integer voxel offsets from the source; a handle's position is lattice(source, voxel, offset)."""

    def __init__(self, device, W: int, ld: int, chmap, voxel: float, radius: int = 4, patch: int = 2):
        self.device = th.device(device)
        self.W, self.ld, self.voxel, self.R, self.rp = int(W), int(ld), float(voxel), int(radius), int(patch)
        cm = np.asarray(chmap.detach().cpu() if th.is_tensor(chmap) else chmap).astype(np.int32).reshape(3, -1)
        if cm.shape[1] < 1 or cm.min() < 0 or cm.max() >= self.ld:
            raise ValueError(f"chmap must be [3][Cc >= 1] with tap channels in 0..{self.ld - 1}")
        self.chmap = th.as_tensor(np.ascontiguousarray(cm)).to(self.device)
        self.Cc = cm.shape[1]
        self._L = _lib.lib()
        if self.W < 2 or self.ld < 1 or self._L.ishap_drag_track_scratch_bytes(1, 1, self.R, self.rp, self.Cc) < 0:
            raise ValueError(f"handle tracker: radius = {radius} (0..8), patch = {patch} (0..4), W = {W} (>= 2), ld = {ld}")
        self.side = 2 * self.R + 1
        self.sources = None

    def setup(self, sources):
        """sources: a list of E handle arrays [B_e, 3] (one per edit).  Allocates the per-call buffers; nothing is launched."""
        src, _, offs = pack_handles(sources, sources)
        self.E = len(offs) - 1
        try:
            self.scratch, nbytes = _lib.scratch(self.device, "ishap_drag_track_scratch_bytes", self.E, offs[-1], self.R, self.rp, self.Cc)
        except _lib.ScratchError:
            raise ValueError(f"handle tracker: {self.E} edits (1..32)") from None
        self.sources, self.offsets = src.to(self.device), list(offs)
        self._offs = (C.c_int * (self.E + 1))(*offs)
        self._chmap_ptr, self._src_ptr = self.chmap.data_ptr(), self.sources.data_ptr()
        self._scratch_ptr, self._scratch_bytes = self.scratch.data_ptr(), nbytes
        return self

    @property
    def handles(self) -> int:
        return self.offsets[-1]

    def run_ptr(self, edit_ptr: int, orig_ptr: int, orig_stride: int, K_in, K_out, dist, dist0, volume=None):
        """One tracking call on the current stream: edit [E][W*W][ld] fp16, guidance edit e at orig + e * orig_stride halfs;
        K_in / K_out int32 [H, 3], dist / dist0 float32 [H], volume None or float32 [H, side^3], all on the device."""
        self.run_raw(edit_ptr, orig_ptr, orig_stride, K_in.data_ptr(), K_out.data_ptr(), dist.data_ptr(), dist0.data_ptr(),
                     _lib.ptr(volume))

    def run_raw(self, edit_ptr: int, orig_ptr: int, orig_stride: int, k_in: int, k_out: int, dist: int, dist0: int, volume=None):
        """run_ptr on device addresses (the guided loop's form: no tensor is made per step)."""
        _lib.call(self.device, "ishap_drag_track", edit_ptr, orig_ptr, int(orig_stride), self.W, self.ld, self.Cc, self._chmap_ptr,
                  self._src_ptr, self._offs, self.E, self.voxel, self.R, self.rp, k_in, k_out, dist, dist0, volume,
                  self._scratch_ptr, self._scratch_bytes)

    def positions(self, offsets: th.Tensor) -> th.Tensor:
        """lattice(source, voxel, K) in float32 (the product rounded, then the sum), for offsets [..., H, 3]."""
        return self.sources + th.tensor(self.voxel, dtype=th.float32, device=self.device) * offsets.to(th.float32)

    def _tap(self, t, lead):
        if t.dtype != th.float16 or tuple(t.shape[-2:]) != (self.W * self.W, self.ld):
            raise ValueError(f"taps are fp16 [..., {self.W * self.W}, {self.ld}], got {t.dtype} {tuple(t.shape)}")
        t = t.to(self.device).contiguous()
        if t.dim() == 2:
            t = t[None]
        if t.dim() != 3 or t.shape[0] not in lead:
            raise ValueError(f"tap batch of {tuple(t.shape)} for {self.E} edits")
        return t

    def track_batch(self, edit_taps, orig_taps, sources, offsets=None, want_volume=False) -> List[Track]:
        """E edits in one call.  edit_taps [E, W*W, ld]; orig_taps [E, W*W, ld] or one [W*W, ld] for all; sources: E handle
        arrays; offsets: None (zeros) or E int arrays [B_e, 3], each handle's last offset.  One Track per edit."""
        self.setup(sources)
        edit, orig = self._tap(edit_taps, (self.E,)), self._tap(orig_taps, (1, self.E))
        H = self.handles
        if offsets is None:
            K_in = th.zeros((H, 3), dtype=th.int32, device=self.device)
        else:
            K_in = th.cat([th.as_tensor(np.asarray(o.detach().cpu() if th.is_tensor(o) else o)).to(th.int32).reshape(-1, 3)
                           for o in offsets]).to(self.device).contiguous()
            if K_in.shape[0] != H:
                raise ValueError(f"{K_in.shape[0]} offsets for {H} handles")
        K_out = th.empty_like(K_in)
        dist, dist0 = th.empty(H, dtype=th.float32, device=self.device), th.empty(H, dtype=th.float32, device=self.device)
        vol = th.empty((H, self.side ** 3), dtype=th.float32, device=self.device) if want_volume else None
        self.run_ptr(edit.data_ptr(), orig.data_ptr(), 0 if orig.shape[0] == 1 else orig[0].numel(), K_in, K_out, dist, dist0, vol)
        pos = self.positions(K_out)
        cut = lambda t, e: None if t is None else t[self.offsets[e]:self.offsets[e + 1]]      # noqa: E731
        return [Track(cut(K_out, e), cut(pos, e), cut(dist, e), cut(dist0, e), cut(vol, e)) for e in range(self.E)]

    def track(self, edit_tap, orig_tap, sources, offsets=None, want_volume=False) -> Track:
        """One edit: taps [W*W, ld] fp16, sources [B, 3], offsets None or int [B, 3] -> Track(offsets int32 [B, 3], positions
        float32 [B, 3], dist [B], dist0 [B], volume [B, side^3] or None)."""
        return self.track_batch(edit_tap, orig_tap, [sources], None if offsets is None else [offsets], want_volume)[0]


class _LoopTrack:
    """The tracking of one guided loop: a device table of offsets, one row per tracked step behind a row of zeros, so that each
    call reads the row before it and no step waits for the host."""

    def __init__(self, tracker: HandleTracker, sources, steps_total: int, every: int):
        self.tracker, self.every = tracker.setup(sources), every
        rows = (steps_total + every - 1) // every
        H, dev = tracker.handles, tracker.device
        self.table = th.zeros((rows + 1, H, 3), dtype=th.int32, device=dev)
        self.dist = th.zeros((rows, H), dtype=th.float32, device=dev)
        self.dist0 = th.zeros((rows, H), dtype=th.float32, device=dev)
        self.steps: List[int] = []
        self._ptrs = (self.table.data_ptr(), self.dist.data_ptr(), self.dist0.data_ptr(), H)

    def step(self, n: int, edit_ptr: int, orig_ptr: int, orig_stride: int):
        if n % self.every:
            return
        r = len(self.steps)
        table, dist, dist0, H = self._ptrs                 # rows r and r + 1 of the table, row r of the distances
        self.tracker.run_raw(edit_ptr, orig_ptr, orig_stride, table + 12 * H * r, table + 12 * H * (r + 1), dist + 4 * H * r,
                             dist0 + 4 * H * r)
        self.steps.append(n)

    def results(self) -> List[dict]:
        """One dict per edit: steps (the loop's step numbers, 0 the first), offsets [rows, B, 3], positions, dist, dist0 [rows, B]."""
        t, r = self.tracker, len(self.steps)
        offs = self.table[1:r + 1].clone()
        pos = t.positions(offs)
        out = []
        for e in range(t.E):
            a, b = t.offsets[e], t.offsets[e + 1]
            out.append({"steps": list(self.steps), "offsets": offs[:, a:b], "positions": pos[:, a:b],
                        "dist": self.dist[:r, a:b].clone(), "dist0": self.dist0[:r, a:b].clone(), "radius": t.R, "patch": t.rp})
        return out


CLOSED_LOOP_DEFAULTS = {"step": 2.0, "arrive": 1.0, "stop": False, "lag": 2}


def _closed_loop_one(cl, what: str) -> dict:
    opts = dict(CLOSED_LOOP_DEFAULTS)
    if cl is not True:
        if not isinstance(cl, dict):
            raise ValueError(f"{what}: None, True or a dict with any of step, arrive, stop, lag (got {type(cl).__name__})")
        unknown = set(cl) - set(opts)
        if unknown:
            raise ValueError(f"{what}: unknown keys {sorted(unknown)} (step, arrive, stop, lag)")
        opts.update(cl)
    try:
        step, arrive = float(opts["step"]), float(opts["arrive"])
    except (TypeError, ValueError):
        raise ValueError(f"{what}: step and arrive must be numbers") from None
    if not step > 0:                      # NaN fails too
        raise ValueError(f"{what}: step = {opts['step']} (the lead in voxels: must be > 0, may be inf)")
    if not arrive >= 0:
        raise ValueError(f"{what}: arrive = {opts['arrive']} (voxels: must be >= 0)")
    if not isinstance(opts["stop"], (bool, np.bool_)):
        raise ValueError(f"{what}: stop = {opts['stop']!r} (must be True or False)")
    lag = opts["lag"]
    if isinstance(lag, (bool, np.bool_)) or not isinstance(lag, (int, np.integer)) or lag < 1:
        raise ValueError(f"{what}: lag = {lag!r} (an integer >= 1: the host looks at the stop flag of `lag` steps ago)")
    return {"step": step, "arrive": arrive, "stop": bool(opts["stop"]), "lag": int(lag)}


def closed_loop_options(closed_loop, K: Optional[int] = None) -> Optional[dict]:
    """The `closed_loop` keyword of training() / training_part() / training_batch(): None or False (off), True (the defaults) or
    a dict with any of step, arrive, stop, lag -> None or the full dict.  With K (training_batch) also a list of K such entries,
    one per edit: step and arrive then come back as lists of K floats; stop and lag belong to the loop and must agree."""
    if closed_loop is None or closed_loop is False:
        return None
    if K is not None and isinstance(closed_loop, (list, tuple)):
        if len(closed_loop) != K:
            raise ValueError(f"closed_loop: {len(closed_loop)} entries for {K} edits (give one value or one per edit)")
        each = [_closed_loop_one(True if c is None else c, f"closed_loop[{k}]") for k, c in enumerate(closed_loop)]
        if any(o["stop"] != each[0]["stop"] or o["lag"] != each[0]["lag"] for o in each):
            raise ValueError("closed_loop: stop and lag belong to the loop: every edit must give the same")
        return {"step": [o["step"] for o in each], "arrive": [o["arrive"] for o in each], "stop": each[0]["stop"], "lag": each[0]["lag"]}
    return _closed_loop_one(closed_loop, "closed_loop")


def closed_loop_track(closed_loop_opts, track):
    """The `track` keyword under a closed loop: tracking is what closes it, so it is on when not given and may not be False."""
    if closed_loop_opts is None:
        return track
    if track is False:
        raise ValueError("closed_loop needs the handle tracking: track may not be False")
    return True if track is None else track


class _ClosedLoop:
    """The re-aiming of one guided loop: after every tracked step one retarget reads the row of offsets the
    tracker just wrote and writes the next row of goals, which the loss calls read from then on.  Row 0 is the retarget on the
    table's row of zeros, run here, before the first step.  The host passes addresses only.
    stop: after each retarget the step's `done` row is copied to pinned memory behind an event; before enqueueing guided step n
    the loop waits for the event of step n - lag -- a fixed step, whatever the timing -- and stops if every edit was done then."""

    def __init__(self, dk, trk: "_LoopTrack", opts: dict):
        self.dk, self.trk, self.opts = dk, trk, opts
        H, E, dev = trk.tracker.handles, trk.tracker.E, trk.tracker.device
        rows = trk.table.shape[0]                     # tracked steps + 1
        self.goals = th.zeros((rows, H, 3), dtype=th.float32, device=dev)
        self.remaining = th.zeros((rows, H), dtype=th.float32, device=dev)
        self.arrived = th.zeros((rows, H), dtype=th.int32, device=dev)
        self.done = th.zeros((rows, E), dtype=th.int32, device=dev)
        self._ptrs = (trk.table.data_ptr(), self.goals.data_ptr(), self.remaining.data_ptr(), self.arrived.data_ptr(),
                      self.done.data_ptr(), H, E)
        self.stop, self.lag = opts["stop"], opts["lag"]
        self.done_host = th.zeros((rows, E), dtype=th.int32).pin_memory() if self.stop else None
        self.events: list = []                        # per loop step n: (event, row) of the newest `done` row at that step
        dk._aim_keep = self.goals                     # the kernels object outlives the loop and keeps aiming at a row of this table
        self._retarget(0)

    def _retarget(self, r: int):
        table, goals, rem, arr, done, H, E = self._ptrs
        self.dk.retarget_raw(table + 12 * H * r, goals + 12 * H * r, rem + 4 * H * r, arr + 4 * H * r, done + 4 * E * r,
                             self.opts["step"], self.opts["arrive"])

    def step(self, n: int):
        """After the tracker's call of step n, on the same stream."""
        tracked = bool(self.trk.steps) and self.trk.steps[-1] == n
        r = len(self.trk.steps)
        if tracked:
            self._retarget(r)
        if self.stop:
            if tracked or not self.events:
                self.done_host[r].copy_(self.done[r], non_blocking=True)
                ev = th.cuda.Event()
                ev.record()
                self.events.append((ev, r))
            else:
                self.events.append(self.events[-1])

    def stop_before(self, n: int) -> bool:
        """Before guided step n is enqueued: was every edit done at step n - lag?"""
        if not self.stop or n < self.lag:
            return False
        ev, r = self.events[n - self.lag]
        ev.synchronize()
        return bool(self.done_host[r].all())

    def results(self, out: List[dict]) -> List[dict]:
        """Adds to the tracker's per-edit dicts: goals [rows, B, 3], remaining [rows, B], arrived [rows, B] (bool), row r what the
        loss of tracked step r aimed at (formed from offsets[r - 1]; zeros for r = 0), and remaining_after [B], arrived_after [B],
        the same after the last tracked step."""
        t, r = self.trk.tracker, len(self.trk.steps)
        for e, d in enumerate(out):
            a, b = t.offsets[e], t.offsets[e + 1]
            d.update(goals=self.goals[:r, a:b].clone(), remaining=self.remaining[:r, a:b].clone(),
                     arrived=self.arrived[:r, a:b] != 0, remaining_after=self.remaining[r, a:b].clone(),
                     arrived_after=self.arrived[r, a:b] != 0, step=per_edit(self.opts["step"], t.E, "step")[e],
                     arrive=per_edit(self.opts["arrive"], t.E, "arrive")[e])
        return out


class VolumeGuidance:
    """The volume constraints of one guided loop (constraints.py): per step the gradient of
    L_vol = -(1 / sum w) sum_j w_j BCEWithLogits(decoder(planes of pred_xstart)(q_j), g_j) with respect to the step's latent,
    composed as DragStuff.reconstruct composes its own -- pred_xstart, prepare_planes, the loss on the planes,
    ishap_x0_grad_to_cotangent, ishap_grad_to_scaled_f16, the full-depth backward, plus the direct route -- and its mix into the
    drag gradient.  The points are fixed for the edit: their gather list is built once (MultiTriplane.constraint_setup)."""

    def __init__(self, ds: "DragStuff", cons, ratio: float):
        self.ds, self.ratio = ds, float(ratio)
        dev, S = ds.device, ds.args.image_size
        self.state = ds.decoder.constraint_setup(cons.points, cons.targets, cons.weights, S)
        self.rng = ds.range.reshape(-1).contiguous() if th.is_tensor(ds.range) else None
        self.dplanes = th.empty((3, S, S, 32), dtype=th.float32, device=dev)
        self.cot = th.empty((1, 192, S, S), dtype=th.float32, device=dev)
        self.cot16 = th.empty((1, 192, S, S), dtype=th.float16, device=dev)
        self.bits = th.zeros(1, dtype=th.int32, device=dev)
        self.scale2 = th.ones(2, dtype=th.float32, device=dev)

    def gradient(self, x, i, model_output, loss_out=None):
        """d L_vol / d x of the step (x, i) whose complete model output is `model_output` and whose forward the model keeps;
        L_vol goes to loss_out (device float[1]).  A full-depth backward: runs after the forward's tail has been joined."""
        ds, d = self.ds, self.ds.diffusion
        dev, S = ds.device, ds.args.image_size
        ti = d._t_index(i)
        # the step kernel with pred_xstart as its only output: the one extra elementwise launch (the guided loop clips, as its step does)
        x0 = d._step(x, model_output, ti, None, None, True, 0, ("pred_xstart",))["pred_xstart"]
        planes = prepare_planes(x0, ds.range, ds.middle)
        ds.decoder.constraint_loss_grad(planes, self.state, dplanes=self.dplanes, loss=loss_out)
        g_direct = th.empty_like(x)
        sr = float(np.float32(d.sqrt_recip_alphas_cumprod[ti]))
        srm1 = float(np.float32(d.sqrt_recipm1_alphas_cumprod[ti]))
        _lib.call(dev, "ishap_x0_grad_to_cotangent", self.dplanes.data_ptr(), _lib.ptr(self.rng), x.data_ptr(), model_output.data_ptr(),
                  sr, srm1, 1, S, g_direct.data_ptr(), self.cot.data_ptr())
        _lib.call(dev, "ishap_grad_to_scaled_f16", self.cot.data_ptr(), self.cot16.data_ptr(), self.bits.data_ptr(),
                  self.scale2.data_ptr(), self.cot.numel())
        dx = ds.model.backward_from_output(self.cot16, self.scale2)
        grad = th.empty_like(dx)
        _lib.call(dev, "ishap_axpby", dx.data_ptr(), g_direct.data_ptr(), 1.0, 1.0, dx.numel(), grad.data_ptr())
        return grad

    def mix(self, grad_drag, grad_vol):
        """grad_drag + (volume_scale / scale) grad_vol: what the guided update multiplies by scale"""
        out = th.empty_like(grad_drag)
        _lib.call(self.ds.device, "ishap_axpby", grad_drag.data_ptr(), grad_vol.data_ptr(), 1.0, self.ratio, grad_drag.numel(),
                  out.data_ptr())
        return out


def synthesize_latent(model, diffusion, args=None, t1=None, t2=0, inter_latent_idx=None, inter_feat_idx=None, img=None,
                      calc_grad=False, **kwargs):
    """drag_utils.py:61-131 (no caller in the reference; kept for the call surface).  calc_grad=True keeps the autograd
    graph from the returned tensors back to `img` (a fresh leaf when `img` is None, :86-87; pass a tensor with
    requires_grad=True otherwise, as there) through differentiable.UNetCall, and records `noise` / `variance` at the
    inter_feat_idx steps (:104-105); calc_grad=False runs the same loop under no_grad (:115-128)."""
    if args is None:
        args = get_args()
    shape = (args.batch_size, 96, args.image_size, args.image_size)
    if img is None:
        img = th.randn(shape, device=next(model.parameters()).device)
        if calc_grad:
            img.requires_grad_(True)
    assert img.shape == shape
    if t1 is None:
        t1 = args.num_steps
    elif t1 == 0:
        return {"img": img[:args.num_samples], "inter_latent": [], "inter_feat": [], "pred_xstart": [], "model_output": None}
    sample_fun = diffusion.ddim_sample if getattr(args, "use_ddim", False) else diffusion.p_sample_guidance
    if calc_grad and getattr(args, "use_ddim", False):
        # only p_sample_guidance routes a requires_grad input through differentiable.UNetCall; ddim_sample would cut the
        # graph silently (the reference keeps it, drag_utils.py:96-113) -- refuse rather than return detached tensors
        raise NotImplementedError("synthesize_latent(calc_grad=True) with use_ddim: the DDIM sampler has no autograd bridge")
    inter_latent, inter_feat, predict_x0, model_output, variance, noise = [], [], [], None, [], []
    with (th.enable_grad() if calc_grad else th.no_grad()):
        for i in range(t1 - 1, t2 - 1, -1):
            out = sample_fun(model, img, i, **kwargs)
            img = out["sample"]
            if inter_feat_idx is not None and i in inter_feat_idx:
                inter_feat.append(out["inter_feat"])
                if calc_grad:
                    noise.append(out["noise"].cpu())
                    variance.append(out["variance"].cpu())
            if inter_latent_idx is not None and i in inter_latent_idx:
                inter_latent.append(img)
                predict_x0.append(out["pred_xstart"])
            model_output = out["model_output"]
    return {"img": img[:args.num_samples], "inter_latent": inter_latent, "inter_feat": inter_feat,
            "pred_xstart": predict_x0, "model_output": model_output, "variance": variance, "noise": noise}


def load_triplane_stats(stats=None, stats_dir=None):
    """(means, stds) of the triplane statistics (96 values each) for train_triplane_opt's init: `stats` when given, else
    {stats_dir}/means.npy and stds.npy (the reference reads them from the chairs statistics directory)."""
    if stats is not None:
        means, stds = stats
    else:
        files = [os.path.join(stats_dir, f) for f in ("means.npy", "stds.npy")] if stats_dir else []
        if not files or not all(os.path.exists(f) for f in files):
            raise FileNotFoundError(
                "train_triplane_opt needs the triplane statistics: pass stats=(means, stds) or set args.stats_dir to a "
                f"directory holding means.npy and stds.npy (stats_dir={stats_dir!r})")
        means, stds = (np.load(f) for f in files)
    means, stds = (np.asarray(v, dtype=np.float32).reshape(-1) for v in (means, stds))
    if means.size != 96 or stds.size != 96:
        raise ValueError(f"triplane statistics must hold 96 values each, not {means.size} and {stds.size}")
    return means, stds


class DragStuff:
    """drag_utils.py:174-583."""

    args = get_args()
    overlap_tail = None       # None: the module default (_OVERLAP_TAIL, i.e. ISHAP_OVERLAP_TAIL); True / False: this object only
    # First-step reuse (training()): every edit of a loaded shape starts from the same latent `w` at the same timestep through the
    # same weights, so the forward of its first guided step -- model output, tap, everything the backward re-reads -- is the same,
    # bit for bit, in every edit.  The first edit takes a snapshot of it (UNetModel.snapshot_save) and keeps the model output;
    # later edits restore it instead of running the model.  `_shape_gen` counts the changes of what that forward depends on.
    _w = None
    _shape_gen = 0
    _first_step = None        # {"key": ..., "out": model output} of the snapshot the model holds

    @property
    def w(self):
        """The latent every edit starts from (timestep w_time).  Assigning it invalidates the first-step snapshot; so does an
        in-place change (the snapshot records the tensor's version counter)."""
        return self._w

    @w.setter
    def w(self, value):
        self._w = value
        self._shape_changed()

    def _shape_changed(self):
        self._shape_gen = self._shape_gen + 1
        self._first_step = None

    def _first_step_key(self, overlap):
        w = self._w
        return (self._shape_gen, id(self.model), id(w), getattr(w, "_version", None), tuple(w.shape), self.args.feat_layer,
                self.args.w_time, tuple(getattr(self.diffusion, "timestep_map", ())), bool(overlap))

    def __init__(self, device=None, args=None, max_edits=1):
        """`max_edits`: the most edits one training_batch call may run (the model context is built for that batch size; the
        default 1 builds exactly the single-edit object)."""
        if args is not None:
            self.args = args
        if int(max_edits) < 1:
            raise ValueError(f"max_edits must be >= 1, not {max_edits}")
        self.max_edits = int(max_edits)
        self.device = th.device("cuda", th.cuda.current_device()) if device is None else th.device(device)
        self.model, self.diffusion = create_model_and_diffusion(
            **args_to_dict(self.args, model_and_diffusion_defaults().keys()), device=self.device, max_batch=self.max_edits)
        self.model.eval()
        self.decoder = MultiTriplane(1, input_dim=3, output_dim=1, device=self.device)
        self.decoder.eval()
        self.range = 1.
        self.middle = 0.
        self.latent_code = None
        self.w0 = None
        self.w = None
        self.r1 = 12
        self.offset1 = make_offsets(self.r1, self.device)
        self.voxel_size = 2. / self.args.shape_resolution
        self.train_flag = True
        self.targets = None
        self.sources = None
        self.mesh = None
        self.mesh0 = None
        self.tri_feat0 = None         # the final latent of the UNEDITED shape [1, 96, S, S] on the device: volume_keep's targets
        self.last_volume_losses: List[th.Tensor] = []    # after an edit with volume constraints: L_vol per step, device scalars
        self.volume = None            # last decoded occupancy-logit volume [res]^3 on the device
        self.clean = None             # None, or volume.clean_volume keywords (e.g. {"keep": "largest"}): get_mesh cleans the volume
        self.refine = None            # None, or {"iterations": n, "max_move": decoder units}: get_mesh puts the smoothed vertices back
                                      # on the decoder's zero level set and keeps its analytic normals (mesh.OccupancyMesh refine)
        self.mesh_resolution = None   # None, or an int above args.shape_resolution (up to 2048): get_mesh returns the surface at THAT
                                      # resolution, cut from bricks near the surface only (mesh.SparseOccupancyMesh) and seeded from the
                                      # shape_resolution volume, which stays `self.volume` for the metrics, regions and parts
        self.mesh_simplify = None     # None, or a cell size in voxels of the mesh's grid (or mesh.OccupancyMesh's simplify dict): get_mesh
                                      # reduces the smoothed mesh by quadric vertex clustering before refine (mesh.simplify_vertex_clustering)
        self.noise = []
        self.variance = []
        self.variance_noise = []
        self.feature_guidance: List[th.Tensor] = []     # fp16 NHWC taps [S*S, C] on the device
        self.last_losses: List[float] = []
        self.last_track = None        # after an edit with track=...: dict of steps / offsets / positions / dist / dist0 (batch: a list)
        self.last_stop = None         # after a closed-loop edit with stop: the guided step it stopped before, or None (ran them all)
        self._dk: Optional[DragKernels] = None
        self.step_noise = None        # optional callable i -> noise tensor (parity runs); default randn like the reference
        # batched edits (training_batch): set by update_latent_params_batch; None = edit variants of the single shape
        self.w_batch = None
        self.w0_batch = None
        self.feature_guidance_batch: List[th.Tensor] = []     # fp16 NHWC taps [K, S*S, C], one per guided step
        self.meshes0 = []
        self.meshes = []
        self.volumes = []

    def set_offset1(self, r1):
        self.r1 = int(r1)
        self.offset1 = make_offsets(r1, self.device)

    # ------------------------------------------------------------------ checkpoints (drag_utils.py:213-249)
    def update_model_params(self, main_path):
        for files in os.listdir(main_path):
            if files.startswith("ddpm"):
                ddpm_path = os.path.join(main_path, files)
                for sub_file in os.listdir(ddpm_path):
                    if sub_file.startswith("ema"):
                        self.args.model_path = os.path.join(ddpm_path, sub_file)
                        break
            elif files.endswith(".pt"):
                self.args.decoder_ckpt = os.path.join(main_path, files)
        stat_path = os.path.join(main_path, "statistics")
        self.args.stats_dir = os.path.join(stat_path, os.listdir(stat_path)[0])
        self.args.save_dir = os.path.join("samples", main_path[9:] + "_samples")
        os.makedirs(self.args.save_dir, exist_ok=True)
        self.load_weights(th.load(self.args.model_path, map_location="cpu"),
                          th.load(self.args.decoder_ckpt, map_location="cpu"),
                          np.load(f"{self.args.stats_dir}/lower_bound.npy") if self.args.explicit_normalization else None,
                          np.load(f"{self.args.stats_dir}/upper_bound.npy") if self.args.explicit_normalization else None)

    def load_weights(self, unet_sd, decoder_sd, lower_bound=None, upper_bound=None):
        """The in-memory half of update_model_params (:229-249)."""
        self._shape_changed()
        self.model.load_state_dict(unet_sd, strict=True)
        if self.args.use_fp16:
            self.model.convert_to_fp16()
        self.model.eval()
        if lower_bound is not None:
            mn = np.asarray(lower_bound).astype(np.float32).reshape(1, -1, 1, 1)
            mx = np.asarray(upper_bound).astype(np.float32).reshape(1, -1, 1, 1)
            self.range = (th.tensor(mx - mn) / 2).to(self.device)
            self.middle = th.tensor((mn + mx) / 2).to(self.device)
        else:
            self.range, self.middle = 1., 0.
        self.decoder.net.load_state_dict(decoder_sd)
        self.decoder.eval()

    # ------------------------------------------------------------------ sampling with guidance cache (:252-280)
    def _noise(self, i, like):
        return None if self.step_noise is None else self.step_noise(i).to(like.device)

    def _denoise(self, img, t, each=None, **kwargs):
        """The unguided steps i = t - 1 .. 0 from `img`; `each(i, sample)` runs after step i.  Returns the last sample."""
        for i in range(t - 1, -1, -1):
            img = self.diffusion.p_sample_guidance(self.model, img, i, feat_layer=self.args.feat_layer,
                                                   clip_denoised=self.args.clip_denoised, want_inter_feat=False,
                                                   noise=self._noise(i, img), want_noise=False, **kwargs)["sample"]
            if each is not None:
                each(i, img)
        return img

    def update_latent_params(self, img=None, **kwargs):
        if img is not None:
            if th.is_tensor(img):
                img = img.type(th.float32).to(self.device)
            elif type(img) is np.ndarray:
                img = th.tensor(img, dtype=th.float32, device=self.device)
            else:
                raise NotImplementedError("Unknown data type!")
        else:
            img = th.randn((1, 96, self.args.image_size, self.args.image_size), dtype=th.float32, device=self.device)
        self.latent_code = img.clone().detach()
        self._shape_changed()
        self.w_batch, self.w0_batch, self.feature_guidance_batch = None, None, []     # training_batch: variants of this shape

        def record(i, img):
            if i == self.args.w_time:
                self.w = img.clone().detach()
                self.w0 = self.w.clone().detach()
            if i < self.args.w_time:
                self.feature_guidance.append(self.model.copy_tap(self.args.feat_layer)[0])

        img = self._denoise(img, self.args.num_steps, each=record, **kwargs)
        assert len(self.feature_guidance) == self.args.w_time
        self.mesh0 = self.get_mesh(tri_feat=img)
        self.tri_feat0 = img.detach().clone()
        self.mesh = copy.deepcopy(self.mesh0)
        return img

    # ------------------------------------------------------------------ decode (:282-300)
    def _sparse_mesh_resolution(self):
        """mesh_resolution when it asks for the sparse path (an int above shape_resolution), else None"""
        r = self.mesh_resolution
        if r is None:
            return None
        if isinstance(r, bool) or int(r) != r or not 9 <= int(r) <= 2048:
            raise ValueError(f"mesh_resolution must be None or an int in 9 .. 2048, not {r!r}")
        if int(r) - 1 > 64 * (self.args.shape_resolution - 1):
            raise ValueError(f"mesh_resolution {r} is too fine for a shape_resolution of {self.args.shape_resolution}: the volume "
                             f"seeds meshes up to {64 * (self.args.shape_resolution - 1) + 1}")
        return int(r) if int(r) > self.args.shape_resolution else None

    def get_mesh(self, tri_feat=None, img=None, t=0):
        if tri_feat is None:
            img = img if img is not None else th.randn((1, 96, self.args.image_size, self.args.image_size)).to(self.device)
            tri_feat = self._denoise(img, t)
        self.tri_feat = tri_feat
        refine = None
        sparse = self._sparse_mesh_resolution()
        if self.refine is None and sparse is None:
            self.volume = decode_volume(self.decoder, tri_feat.to(self.device), self.range, self.middle,
                                        self.args.shape_resolution)
        else:                         # decode_volume's two halves, keeping the planes for the projection (get_meshes comes here too)
            planes = prepare_planes(tri_feat.to(self.device), self.range, self.middle)
            self.volume = decode_planes_grid(self.decoder, planes, self.args.shape_resolution)
            refine = None if self.refine is None else dict(self.refine, decoder=self.decoder, planes=planes)
        if self.clean is not None:    # floaters / cavities out before the surface; self.volume is then the cleaned volume
            self.volume = clean_volume(self.volume, **self.clean)
        if sparse is not None:        # the volume decoded anyway seeds the bricks of the fine grid
            return mesh_backend.sparse_volume_to_mesh(self.decoder, planes, sparse, self.volume, smooth_iterations=10, refine=refine,
                                                      simplify=self.mesh_simplify)
        return mesh_backend.volume_to_mesh(self.volume, self.args.shape_resolution, smooth_iterations=10, refine=refine,
                                           simplify=self.mesh_simplify)

    # ------------------------------------------------------------------ drag loop (:302-399)
    def _guided_loop(self, img, dk, guidance, stride, scales, guided_scale, reuse_first=False, trk=None, cl=None, vol=None):
        """The guided loop of training() and training_batch(): a generator that yields the progress value after each step and
        returns (img, stop_time) -- the latent and the number of unguided steps left when train_flag stopped it (0: ran to
        the end).  `dk`: a DragKernels or BatchDragKernels after setup; `guidance[n]`: the guidance tap of the n-th step, edit e's
        at + e * stride halfs; `scales`: the guidance scale of every image as floats; `guided_scale`: the same as
        p_sample_guidance takes it (a float, or a device tensor with one value per image).  last_losses gets one [images]
        tensor per step.
        `reuse_first` (training() only: `img` is a copy of self.w): the first step's forward comes from the snapshot of an earlier
        edit of this shape when there is a valid one, and is saved as one otherwise.
        `trk`: None, or the _LoopTrack of a tracked edit: its call follows the loss's on the same stream and only reads the tap.
        `cl`: None, or the _ClosedLoop of a closed-loop edit (needs `trk`): its retarget follows the tracker's call, so the order on
        the stream is loss(n), track(n), retarget(n), backward(n); with stop it may clear train_flag before a step (last_stop).
        `vol`: None, or the VolumeGuidance of an edit with volume constraints (training() only, one image): once the model output
        is complete (p_sample_guidance's after_tail) the step adds (volume_scale / scale) d L_vol / d x to the drag gradient -- a
        second, full-depth backward on the same forward -- and last_volume_losses gets one device scalar per step.  Such an edit
        runs with reuse_first=False: a restored snapshot holds the network up to the tap only."""
        w_time = self.args.w_time
        assert vol is None or not reuse_first
        vol_losses = None if vol is None else th.zeros(w_time, dtype=th.float32, device=self.device)
        self.last_volume_losses = []
        overlap = _OVERLAP_TAIL if self.overlap_tail is None else self.overlap_tail
        reuse_first = reuse_first and _FIRST_STEP_REUSE and hasattr(self.model, "snapshot_restore")
        stop_time = 0
        self.train_flag = True
        self.last_stop = None
        losses = th.zeros((w_time, len(scales)), dtype=th.float32, device=self.device)   # one slot per iteration, no per-step copy
        self.diffusion.prepare(self.model, range(w_time))                               # timestep embeddings of the whole loop, once
        self.last_losses = []
        for i in range(w_time - 1, -1, -1):
            if cl is not None and self.train_flag and cl.stop_before(w_time - 1 - i):
                self.train_flag, self.last_stop = False, w_time - 1 - i
            if not self.train_flag:
                stop_time = i + 1
                break
            origin = guidance[w_time - 1 - i]
            slot = losses[i]
            got = {}

            def loss_and_backward():          # needs the tap only
                cot, scale2 = dk.loss_cotangent_ptr(self.model.tap_ptr(), origin.data_ptr(), orig_stride=stride, loss_out=slot)
                if trk is not None:
                    trk.step(w_time - 1 - i, self.model.tap_ptr(), origin.data_ptr(), stride)
                    if cl is not None:
                        cl.step(w_time - 1 - i)
                got["grad"] = self.model.backward_input(cot, scale2)           # = img.grad of the reference (:384)
                return got["grad"]

            # loss + backward run beside the part of the forward after the tap (p_sample_guidance's `between`; ISHAP_OVERLAP_TAIL=0:
            # the plain sequence).  Rounds 2-4 measured a LOSS with whole-layer grids (the tail's 128x128-tile convolutions hold
            # every CU's LDS for a tile's length and the backward chain queues behind them).  Round 5: the tail's convolutions run as
            # launches of at most 64-128 tiles (csrc/igemm4.hip launch4), and -- late round 5 -- the forward only plans them: they are
            # enqueued (model.run_tail, inside p_sample_guidance) behind an event the backward records after its first 16x16 block,
            # so they run beside the backward's latency-bound middle: -3.8 % per edit against the plain sequence
            # (profiles/round5_overlap_tail_ab.txt); bit-identical results, tested.
            # the update img = sample + variance * scale * grad (:384-392) is formed by the step kernel (guided_scale): the loss +
            # backward run between the model call and the step arithmetic either way, beside the forward tail when overlapping
            first = {}
            if reuse_first and i == w_time - 1:
                key, kept = self._first_step_key(overlap), self._first_step
                # restore() is False while the per-launch profile records: that edit runs (and counts) all its forwards
                if kept is not None and kept["key"] == key and self.model.has_snapshot() and self.model.snapshot_restore():
                    first["model_output"] = kept["out"]
                else:
                    def keep_first(mo, key=key):       # after the tail: the model output is complete
                        if self.model.snapshot_save():
                            self._first_step = {"key": key, "out": mo.clone()}
                    first["after_tail"] = keep_first
            if vol is not None:
                def add_volume(mo, x=img, i=i):        # after the tail: pred_xstart needs the whole model output
                    got["grad"] = vol.mix(got["grad"], vol.gradient(x, i, mo, vol_losses[i:i + 1]))
                    return got["grad"]
                first["after_tail"] = add_volume
            outs = self.diffusion.p_sample_guidance(self.model, img, i, feat_layer=self.args.feat_layer,
                                                    keep_for_backward=True, want_inter_feat=False,
                                                    noise=self._noise(i, img), between=loss_and_backward,
                                                    overlap=overlap,
                                                    guided_scale=guided_scale if _FUSED_UPDATE else None, want_noise=False,
                                                    **first)
            if _FUSED_UPDATE:
                img = outs["guided"]
            else:
                new = th.empty_like(img)
                n1 = img[0].numel()
                for k, sc in enumerate(scales):
                    _lib.call(self.device, "ishap_guided_update", outs["sample"][k].data_ptr(), outs["variance"][k].data_ptr(),
                              got["grad"][k].data_ptr(), sc, None, n1, new[k].data_ptr())
                img = new
            self.last_losses.append(slot)
            if vol is not None:
                self.last_volume_losses.append(vol_losses[i])
            yield 1 - i / (w_time - 1.)
        return img, stop_time

    def _region_weights(self, width, cof, keep, free, keep_weight, free_weight, region_dilate, weights, what="cof", region_falloff=0.0):
        """The weight map of one edit's preservation term, or None: `weights` (a ready [3, W, W] map) or the map of the keep /
        free regions (regions.plane_weights at the tap's width).  Everything is validated before anything is launched."""
        from . import regions
        if weights is not None and (keep is not None or free is not None):
            raise ValueError("weights is a ready map: give it or keep / free regions, not both")
        region_falloff = regions.check_falloff(region_falloff)
        has = weights is not None or keep is not None or free is not None
        check_region_cof(float(cof), has, what)
        if weights is not None:
            return check_weight_map(weights, width)
        if not has:
            return None
        return regions.plane_weights(keep=keep, free=free, W=width, keep_weight=keep_weight, free_weight=free_weight,
                                     dilate=region_dilate, device=self.device, falloff=region_falloff)

    def _volume_constraints(self, scale, volume_keep, carve, fill, volume_scale, volume_points, volume_res):
        """-> (constraints.VolumeConstraints, volume_scale / scale), or (None, 0.0) when the edit has none: no region given, or
        volume_scale = 0.  Everything is validated before the edit launches anything."""
        if volume_keep is None and carve is None and fill is None:
            return None, 0.0
        from . import constraints
        from .triplane_decoder import field_grad_planes
        vs = float(scale) if volume_scale is None else float(volume_scale)
        if not np.isfinite(vs):
            raise ValueError(f"volume_scale must be finite, got {volume_scale!r}")
        roles = constraints.check_builder_args(volume_keep, carve, fill, volume_res, volume_points, (1.0, 1.0, 1.0))[0]
        if vs == 0.0:
            return None, 0.0
        if float(scale) == 0.0:
            raise ValueError("scale = 0 with volume constraints: the guided update multiplies the whole gradient by scale, so "
                             "volume_scale / scale has no value")
        ref = None
        if roles[0]:
            if self.tri_feat0 is None:
                raise ValueError("volume_keep needs the unedited shape: load one first (update_latent_params, latent_inversion, "
                                 "train_triplane)")
            planes0 = prepare_planes(self.tri_feat0, self.range, self.middle)
            ref = lambda p: field_grad_planes(self.decoder, planes0, p).logits      # noqa: E731
        cons = constraints.volume_constraints(keep=volume_keep, carve=carve, fill=fill, reference_logits_fn=ref, D=int(volume_res),
                                              max_points=int(volume_points), device=self.device)
        return cons, vs / float(scale)

    def _loop_track(self, topts, width, ch, sources):
        """The tracking state of one guided loop, or None when tracking is off."""
        if topts is None:
            return None
        tracker = HandleTracker(self.device, W=width, ld=ch, chmap=feat_channel_map(ch), voxel=self.voxel_size,
                                radius=topts["radius"], patch=topts["patch"])
        return _LoopTrack(tracker, sources, self.args.w_time, topts["every"])

    def handle_error(self):
        """How far the last tracked edit brought each handle: {"error": |last tracked position - target| in voxels [B],
        "fraction": the share of the requested move covered, (position - source) . (target - source) / |target - source|^2 [B]
        (1 where no move was requested)}; a list of such dicts after training_batch.  Raises if no tracked edit has run."""
        if self.last_track is None:
            raise RuntimeError("handle_error: no tracked edit has run (training(..., track=True))")
        tracks = self.last_track if isinstance(self.last_track, list) else [self.last_track]
        out = []
        for tr, (src, tgt) in zip(tracks, self._track_ends):
            if len(tr["steps"]) == 0:
                raise RuntimeError("handle_error: the tracked edit stopped before its first tracked step")
            pos, move = tr["positions"][-1], tgt - src
            m2 = (move * move).sum(-1)
            frac = th.where(m2 > 0, ((pos - src) * move).sum(-1) / m2.clamp_min(1e-30), th.ones_like(m2))
            out.append({"error": (pos - tgt).norm(dim=-1) / self.voxel_size, "fraction": frac})
        return out if isinstance(self.last_track, list) else out[0]

    def training(self, sources=None, targets=None, scale=600, cof=0.2, keep=None, free=None, keep_weight=4.0, free_weight=0.0,
                 region_dilate=0, weights=None, track=None, closed_loop=None, region_falloff=0.0, volume_keep=None, carve=None,
                 fill=None, volume_scale=None, volume_points=16384, volume_res=128):
        """One drag edit of the loaded shape (drag_utils.py:302-399).  Every edit starts from self.w: from the second edit of a
        shape on, the first guided step's forward is restored from a snapshot instead of run (ISHAP_FIRST_STEP_REUSE=0: always
        run); results are bit-identical either way.
        keep / free: 3-D regions (regions.Box / Sphere / Voxels or lists of them, in the handles' coordinates) whose shadows on
        the three planes get keep_weight (default 4: held harder) / free_weight (default 0: free to change) in the preservation
        term instead of 1, each shadow grown by region_dilate texels; keep overrides free.  region_falloff > 0 (texels) feathers
        the edges of the map over that distance instead of a jump (regions.plane_weights, falloff).  weights: a ready [3, W, W] map
        instead (W the side of the tap), exclusive with keep and free.  All of them need cof > 0.  A plane texel stands for a
        whole column through the shape, so a region constrains its three shadows, not only its own volume.
        track: None (off: no launch is added), True, or {"radius": R, "patch": rp, "every": m}: after every m-th step's loss the
        handles are re-found in feature space (HandleTracker) without a host synchronisation; afterwards last_track holds the
        tracks and handle_error() the distance of each handle's last position to its target.  The edit's results do not change.
        closed_loop: None (off: no launch is added), True, or {"step": 2.0, "arrive": 1.0, "stop": False, "lag": 2} (DESIGN.md
        5.2m): after every tracked step the loss is re-aimed at a goal `step` voxels from each handle's tracked position towards
        its target (the target itself once within `step`), and the touched sets and the preservation term's normalisation follow
        the goals.  Turns tracking on when track is not given.  last_track then also holds goals, remaining and arrived per tracked
        step.  stop: once every handle was within `arrive` voxels of its target `lag` steps ago, the edit finishes with unguided
        steps (last_stop: the step it stopped before).  step = inf is the open-loop edit, bit for bit.
        volume_keep / carve / fill: 3-D regions (Box / Sphere / Voxels of grid size volume_res, or lists) constrained IN THE
        VOLUME, through the decoder (constraints.py): at up to volume_points voxel centres per role of a
        [volume_res]^3 grid the decoded occupancy of every step's pred_xstart is pushed towards that of the unedited shape
        (volume_keep), towards empty (carve) or towards solid (fill); carve and fill override volume_keep, and a voxel in both is a
        ValueError.  The update becomes sample + variance (scale grad_drag + volume_scale grad_vol); volume_scale defaults to
        scale.  With no region, or volume_scale = 0, nothing is launched and the edit is the one it always was, bit for bit;
        constraints with scale = 0 are a ValueError.  A constrained edit costs one full-depth backward more per step and neither
        uses nor takes the first-step snapshot (an earlier one stays valid).  last_volume_losses: L_vol of every step, device
        scalars.  track and closed_loop work as without constraints."""
        yield from self._edits([sources], [targets], [scale], [cof], [keep], [free], [keep_weight], [free_weight], [region_dilate],
                               [weights], track, closed_loop, [region_falloff], one=True,
                               volume=(volume_keep, carve, fill, volume_scale, volume_points, volume_res))

    def _edits(self, sources, targets, scale, cof, keep, free, keep_weight, free_weight, region_dilate, weights, track, closed_loop,
               region_falloff, one=False, volume=None):
        """The edit of training() and training_batch(): K edits in one guided loop, the arguments as training_batch() takes them.
        `one`: training()'s edit -- the single shape (self.w), a single closed_loop setting, a DragKernels kept as self._dk, the
        float guidance scale (the single-scale step kernel), the first-step reuse, `volume` (the arguments of _volume_constraints
        after scale), and afterwards self.sources / self.targets, last_track as one dict and get_mesh."""
        if one and self.args.num_samples > 1:
            raise NotImplementedError("We can handle only one shape at each time!")
        if len(sources) != len(targets):
            raise ValueError(f"{len(sources)} source sets but {len(targets)} target sets: one of each per edit")
        K = len(sources)
        copts = closed_loop_options(closed_loop, None if one else K)
        topts = track_options(closed_loop_track(copts, track))
        check_edit_count(K, self.max_edits)
        scales = per_edit(scale, K, "scale")
        cofs = per_edit(cof, K, "cof")
        ch, width = self.model.tap_shape(self.args.feat_layer)
        keeps, frees, maps = (per_edit_region(v, K, n) for v, n in ((keep, "keep"), (free, "free"), (weights, "weights")))
        kws, fws = per_edit(keep_weight, K, "keep_weight"), per_edit(free_weight, K, "free_weight")
        dils = per_edit_any(region_dilate, K, "region_dilate")
        falls = per_edit_any(region_falloff, K, "region_falloff")
        wmaps = [self._region_weights(width, cofs[k], keeps[k], frees[k], kws[k], fws[k], dils[k], maps[k], "cof" if one else f"cof[{k}]",
                                      falls[k]) for k in range(K)]
        cons, ratio = self._volume_constraints(scales[0], *volume) if one else (None, 0.0)
        if self.w_batch is not None and not one:
            if self.w_batch.shape[0] != K:
                raise ValueError(f"{K} edits for the {self.w_batch.shape[0]} shapes of update_latent_params_batch")
            img = self.w_batch.clone().detach()
            guidance, stride = self.feature_guidance_batch, width * width * ch
        else:
            if self.w is None:
                raise RuntimeError("an edit needs update_latent_params (variants of one shape) or update_latent_params_batch first")
            img = self.w.clone().detach() if one else self.w.expand(K, *self.w.shape[1:]).contiguous()
            guidance, stride = self.feature_guidance, 0
        dims = dict(W=width, ld=ch, chmap=feat_channel_map(ch), r=self.r1, voxel=self.voxel_size, loss_type=self.args.loss_type)
        # an edit without regions makes the call it always made: setup(sources, targets, cof)
        regions = {} if all(w is None for w in wmaps) else {"weights": wmaps[0] if one else wmaps}
        if one:           # the handles go up once, here; the kernels object takes them where they are
            self.sources = th.tensor(np.asarray(sources[0]), device=self.device, dtype=th.float32)
            self.targets = th.tensor(np.asarray(targets[0]), device=self.device, dtype=th.float32)
            dk = self._dk = DragKernels(self.device, **dims)
            dk.setup(self.sources, self.targets, cofs[0], **regions)
        else:
            dk = self._dk_batch = BatchDragKernels(self.device, K, **dims)
            dk.setup(sources, targets, cofs, **regions)
        trk = self._loop_track(topts, width, ch, sources)
        cl = None if copts is None else _ClosedLoop(dk, trk, copts)       # runs the retarget on the tracker's row of zeros
        # the regions change the loss, not the forward: the first-step snapshot depends on the latent, the timestep and the weights
        # of the model only, so _first_step_key does not hold them and an edit with regions reuses the snapshot of a plain one
        # volume constraints need a full-depth backward, which a restored snapshot cannot give: that edit runs its first forward
        vol = None if cons is None else VolumeGuidance(self, cons, ratio)
        guided_scale = scales[0] if one else th.tensor(scales, dtype=th.float32, device=self.device)
        img, stop_time = yield from self._guided_loop(img, dk, guidance, stride, scales, guided_scale, one and vol is None, trk, cl, vol)
        if trk is not None:
            res = trk.results() if cl is None else cl.results(trk.results())
            self.last_track = res[0] if one else res
            self._track_ends = [(dk.sources[a:b], dk.targets[a:b]) for a, b in zip(dk.offsets[:-1], dk.offsets[1:])]
        if one:
            self.mesh = self.get_mesh(img=img, t=stop_time)
        else:
            self.get_meshes(img=img, t=stop_time)

    def training_part(self, part, rigid, handles=16, start=None, scale=600, cof=0.2, keep=None, keep_weight=4.0, free_weight=0.0,
                      region_dilate=0, track=None, closed_loop=None, margin=0.0, region_falloff=0.0, solid=False, volume_scale=None,
                      volume_points=16384):
        """A part edit: move `part` (a regions.Voxels, e.g. from regions.select_part) by `rigid` (a regions.Rigid).  The plan --
        regions.plan_part_edit: `handles` sources spread over the part from `start`, each one's target where the motion takes
        it, free = [the part, the part moved] -- is kept as self.part_plan, and the edit is the generator
        training(plan.sources, plan.targets, scale, cof, keep=keep, free=plan.free, ...), bit for bit.
        Each handle's lattice only translates; a rotation is carried by the handles' different displacements.  r1 stays as
        set_offset1 left it: plan.spacing / voxel_size, the handles' spacing in voxels, is the natural lattice radius to compare
        it with (lattices much smaller leave gaps between handles, much larger ones overlap and average the rotation away).
        margin (voxels): the two free regions are grown by it in 3-D (regions.grow), so that the surface which blends the moved
        part into the rest may change too; region_falloff: as training().  margin = 0 and region_falloff = 0 are the edit it
        always was.  The free regions, like all regions and however grown or feathered, constrain their three shadows, not only
        their volume.  track, closed_loop: as training().
        solid=True adds volume constraints on the part's own grid (training(): carve, fill, volume_scale, volume_points): the place
        the part moves to must fill (fill = plan.moved) and what it leaves must clear (carve = part & ~moved; none when the moved
        part covers the part).  self.part_solid then holds that pair as {"fill": Voxels, "carve": Voxels or None}."""
        from . import regions
        self.part_plan = plan = regions.plan_part_edit(part, rigid, handles=handles, start=start, margin=margin)
        self.part_solid = None
        vkw = {}
        if solid:
            left = part.mask.to(plan.moved.mask.device) & ~plan.moved.mask
            self.part_solid = {"fill": plan.moved, "carve": regions.Voxels(left) if bool(left.any()) else None}
            vkw = dict(fill=plan.moved, carve=self.part_solid["carve"], volume_scale=volume_scale, volume_points=volume_points,
                       volume_res=part.D)
        return self.training(plan.sources, plan.targets, scale=scale, cof=cof, keep=keep, free=plan.free, keep_weight=keep_weight,
                             free_weight=free_weight, region_dilate=region_dilate, region_falloff=region_falloff, track=track,
                             closed_loop=closed_loop, **vkw)

    # ------------------------------------------------------------------ batched edits: K drag edits in one guided loop
    def update_latent_params_batch(self, imgs, **kwargs):
        """update_latent_params for K shapes at once: imgs [K, 96, S, S].  Records w_batch [K, ...], one [K, S*S, C] guidance tap
        per guided step (feature_guidance_batch) and meshes0 (K meshes).  training_batch then edits shape k with edit k."""
        if type(imgs) is np.ndarray:
            imgs = th.tensor(imgs)
        if not th.is_tensor(imgs) or imgs.dim() != 4:
            raise ValueError("update_latent_params_batch: imgs must be a [K, C, S, S] tensor or array")
        K = imgs.shape[0]
        check_edit_count(K, self.max_edits)
        img = imgs.to(device=self.device, dtype=th.float32).contiguous()
        self.latent_code = img.clone().detach()
        self._shape_changed()
        self.feature_guidance_batch = []

        def record(i, img):
            if i == self.args.w_time:
                self.w_batch = img.clone().detach()
                self.w0_batch = self.w_batch.clone().detach()
            if i < self.args.w_time:
                self.feature_guidance_batch.append(self.model.copy_tap(self.args.feat_layer, K))

        img = self._denoise(img, self.args.num_steps, each=record, **kwargs)
        assert len(self.feature_guidance_batch) == self.args.w_time
        self.meshes0 = [self.get_mesh(tri_feat=img[k:k + 1]) for k in range(K)]
        self.meshes = copy.deepcopy(self.meshes0)
        return img

    def get_meshes(self, img, t=0):
        """get_mesh for a batch of latents: the t remaining unguided steps at batch K, then one decode per shape (sets
        tri_feat_batch, volumes, meshes)."""
        img = self._denoise(img, t)
        self.tri_feat_batch = img
        self.meshes, self.volumes = [], []
        for k in range(img.shape[0]):
            self.meshes.append(self.get_mesh(tri_feat=img[k:k + 1]))
            self.volumes.append(self.volume)
        return self.meshes

    def training_batch(self, sources, targets, scale=600, cof=0.2, keep=None, free=None, keep_weight=4.0, free_weight=0.0,
                       region_dilate=0, weights=None, track=None, closed_loop=None, region_falloff=0.0, volume_keep=None, carve=None,
                       fill=None, volume_scale=None):
        """K drag edits in one guided loop (the generator of training(), same progress values).  sources / targets: lists of K
        handle arrays (their counts may differ); scale, cof: a float or K values.  keep, free, keep_weight, free_weight,
        region_dilate, region_falloff, weights: as training(), one value for every edit or a list of K (entries of keep / free / weights may be
        None: that edit has no such region and, if none at all, the bits of its plain batched edit; a region that is itself a
        list goes inside the list of K).  After update_latent_params_batch edit k
        drags shape k; otherwise the K edits are variants of the single shape of update_latent_params (its w and guidance
        features, shared).  train_flag stops all edits at one stop_time; each then finishes its remaining steps unguided.
        Afterwards: meshes / volumes (K of each) and last_losses (one [K] tensor per step).  Every edit's drag loss and gradient
        are bitwise those of a solo call; the loss scale of the fp16 backward is one power of two for the batch (exact for the
        linear backward).  Injected noise (step_noise -> [K, ...]) makes edit k repeat a solo run with noise k; drawn noise spans
        the batch and differs from a solo run's.
        Every step runs its forward: the first-step snapshot of training() is neither used nor taken here.
        track: as training(), one setting for all edits and one launch pair per tracked step; last_track is then a list of K.
        closed_loop: as training(), one dict for all edits or a list of K (step and arrive per edit; stop and lag must agree): one
        retarget launch per tracked step for all edits; with stop the loop stops once EVERY edit was done.
        volume_keep, carve, fill, volume_scale (training()'s volume constraints) are not available for batched edits:
        NotImplementedError."""
        if any(v is not None for v in (volume_keep, carve, fill, volume_scale)):
            raise NotImplementedError("volume constraints (volume_keep, carve, fill, volume_scale) are not available in training_batch: "
                                      "run such an edit with training()")
        yield from self._edits(sources, targets, scale, cof, keep, free, keep_weight, free_weight, region_dilate, weights, track,
                               closed_loop, region_falloff)

    # ------------------------------------------------------------------ real shapes (:401-471, :552-566)
    def _cloud_samples(self, cloud, center, generator=None):
        """occupancy samples of a point cloud ((points, normals), bare points or an .npz path) by winding number; a cloud
        without normals gets them from mesh.estimate_normals inside sample_cloud_occupancy"""
        pts, nrm = mesh_backend.load_cloud(cloud)
        return mesh_backend.sample_cloud_occupancy(pts, nrm, self.args.points_size, self.args.points_uniform_ratio, center=center,
                                                   generator=generator, device=self.device)

    def train_triplane(self, mesh=None, mesh_path=None, center_mesh=True, tri_feat_path=None, path="./",
                       points=None, occupancies=None, occupancy="parity", cloud=None):
        """drag_utils.py:401-471.  `points`/`occupancies` (float32 [P,3] / [P,1]) replace the Open3D raycast
        sampling (:418-440) when given; the mesh-file route needs Open3D like the reference.  occupancy: how the mesh's
        samples are labelled, "parity" or "winding" (mesh.sample_occupancy; "winding" for meshes that are not watertight).
        cloud: a point cloud, labelled by its winding number instead of a mesh (mesh.sample_cloud_occupancy; `center_mesh`
        applies to its points): a (points, normals) pair with unit outward normals, or the path of an .npz with those arrays;
        or points alone -- a [N,3] array or tensor, (points, None), or an .npz without `normals` -- whose normals are then
        estimated and oriented on the device (mesh.estimate_normals, 12 neighbours)."""
        mesh_backend._check_choice("occupancy", occupancy, mesh_backend.OCCUPANCY_METHODS)
        if tri_feat_path is not None:
            img = th.tensor(np.load(tri_feat_path), device=self.device)
            if img.dim() == 3:        # a CHW file (generate.py's triplanes/{i}.npy layout): the model wants a batch axis
                img = img.unsqueeze(0)
            self.mesh = self.get_mesh(img)
            self.mesh0 = copy.deepcopy(self.mesh)
            self.tri_feat0 = img.detach().to(self.device).clone()
            self.latent_inversion(tri_feat=img)
            return
        if points is None and cloud is not None:
            points, occupancies = self._cloud_samples(cloud, center_mesh)
        if points is None:
            points, occupancies = mesh_backend.sample_occupancy(mesh, mesh_path, center_mesh, self.args.points_size,
                                                                self.args.points_uniform_ratio, device=self.device,
                                                                occupancy=occupancy)
            if points is None:
                return
        points = th.as_tensor(np.asarray(points), dtype=th.float32).to(self.device)
        occupancies = th.as_tensor(np.asarray(occupancies), dtype=th.float32).reshape(-1).to(self.device)
        img = self.reconstruct(points, occupancies)
        np.save(os.path.join(path, "tri_feat.npy"), img.cpu().numpy())
        self.clear_params()
        self.mesh = self.get_mesh(tri_feat=img)
        self.mesh0 = copy.deepcopy(self.mesh)
        self.tri_feat0 = img.detach().clone()
        mesh_backend.write_mesh(os.path.join(path, "mesh_recon.obj"), self.mesh0)
        self.latent_inversion(tri_feat=img)

    def reconstruct(self, points, occupancies, scale=600, batch_size=40000, img=None, batch_fn=None, steps=None):
        """The guided-sampling loop of train_triplane (drag_utils.py:442-463): every step decodes `pred_xstart` on a
        random batch of occupancy samples and pushes the latent along d(-BCE)/d img (full-depth UNet backward).
        `batch_fn(i) -> (coord, gt)`, `img` and `steps` (step indices to run) replace the random batch / initial noise /
        full schedule for parity runs.  Every step runs its forward (no first-step snapshot: the input differs from call to
        call); the snapshot training() keeps of the loaded shape stays valid."""
        d = self.diffusion
        if img is None:
            img = th.randn((1, 96, self.args.image_size, self.args.image_size), dtype=th.float32, device=self.device)
        img = img.to(self.device).float().contiguous()
        rng_t = self.range if th.is_tensor(self.range) else None
        S = self.args.image_size
        bits = th.zeros(1, dtype=th.int32, device=self.device)
        scale2 = th.ones(2, dtype=th.float32, device=self.device)
        self.last_losses = []
        for i in (steps if steps is not None else range(self.args.num_steps - 1, -1, -1)):
            outs = d.p_sample_guidance(self.model, img, i, keep_for_backward=True, noise=self._noise(i, img), want_noise=False)
            if batch_fn is not None:
                coord, gt = batch_fn(i)
            else:     # DataLoader(shuffle=True, batch_size=40000); next(iter(...)) -> a fresh random batch each step (:453)
                idx = th.randperm(points.shape[0], device=self.device)[:batch_size]
                coord, gt = points[idx], occupancies[idx]
            from .triplane_decoder import prepare_planes
            planes = prepare_planes(outs["pred_xstart"], self.range, self.middle)
            loss, dplanes, _ = self.decoder.points_loss_grad(planes, coord, gt)
            g_direct = th.empty_like(img)
            cot = th.empty((1, 192, S, S), dtype=th.float32, device=self.device)
            sr = float(np.float32(d.sqrt_recip_alphas_cumprod[i]))
            srm1 = float(np.float32(d.sqrt_recipm1_alphas_cumprod[i]))
            new = th.empty_like(img)
            cot16 = th.empty((1, 192, S, S), dtype=th.float16, device=self.device)
            _lib.call(self.device, "ishap_x0_grad_to_cotangent", dplanes.data_ptr(),
                      _lib.ptr(rng_t.reshape(-1).contiguous()) if rng_t is not None else None, img.data_ptr(),
                      outs["model_output"].data_ptr(), sr, srm1, int(self.args.clip_denoised), S, g_direct.data_ptr(), cot.data_ptr())
            _lib.call(self.device, "ishap_grad_to_scaled_f16", cot.data_ptr(), cot16.data_ptr(), bits.data_ptr(), scale2.data_ptr(),
                      cot.numel())
            dx = self.model.backward_from_output(cot16, scale2)
            grads1 = th.empty_like(dx)                               # = img.grad of the reference (:459): UNet path + direct path
            _lib.call(self.device, "ishap_axpby", dx.data_ptr(), g_direct.data_ptr(), 1.0, 1.0, dx.numel(), grads1.data_ptr())
            _lib.call(self.device, "ishap_guided_update", outs["sample"].data_ptr(), outs["variance"].data_ptr(), grads1.data_ptr(),
                      float(scale), None, img.numel(), new.data_ptr())
            img = new
            self.last_losses.append(loss)
        return img

    def train_triplane_opt(self, mesh=None, mesh_path=None, center_mesh=True, path="./", points=None, occupancies=None,
                           stats=None, epochs=20, batch_size=40000, lr=1e-3, seed=None, batch_fn=None, occupancy="parity",
                           cloud=None):
        """drag_utils.py:473-550: fit the three planes to the mesh's occupancy directly (Adam on BCE + 0.3 pair mse +
        0.001 l2reg + 0.01 tvreg, the MLP frozen; no diffusion model).  `points`/`occupancies` replace the mesh sampling;
        `stats=(means, stds)` replaces {args.stats_dir}/means.npy, stds.npy (the init is randn * stds + means); `seed`
        seeds the one device generator behind the init, the per-epoch permutations and the random pairs;
        `batch_fn(step) -> (idx, r, noise)` injects a step's batch.  Saves tri_feat_opt.npy and mesh_opt.obj under `path`,
        leaves the fitted planes in decoder.embeddings and the per-step (bce, mse, l2reg, tvreg) in last_losses [steps, 4],
        and returns the normalised latent (planes - middle) / range [1,96,S,S].  The drag state is not touched.
        `occupancy` ("parity" | "winding") and `cloud` as train_triplane: how a mesh's samples are labelled, or a
        point cloud, with normals or without, to label instead of a mesh."""
        from .triplane_decoder import fit_triplanes, planes_to_latent
        mesh_backend._check_choice("occupancy", occupancy, mesh_backend.OCCUPANCY_METHODS)
        means, stds = load_triplane_stats(stats, self.args.stats_dir)
        sample_gen = None if seed is None else th.Generator().manual_seed(int(seed))   # a seeded call samples from it
        if points is None and cloud is not None:
            points, occupancies = self._cloud_samples(cloud, center_mesh, sample_gen)
        if points is None:
            points, occupancies = mesh_backend.sample_occupancy(
                mesh, mesh_path, center_mesh, self.args.points_size, self.args.points_uniform_ratio, device=self.device,
                generator=sample_gen, occupancy=occupancy)
            if points is None:
                return None
        points = th.as_tensor(np.asarray(points) if not th.is_tensor(points) else points, dtype=th.float32).to(self.device)
        occupancies = th.as_tensor(np.asarray(occupancies) if not th.is_tensor(occupancies) else occupancies,
                                   dtype=th.float32).reshape(-1).to(self.device)
        S = self.args.image_size
        gen = th.Generator(device=self.device)
        if seed is not None:
            gen.manual_seed(int(seed))
        else:
            gen.seed()
        mean = th.as_tensor(np.asarray(means), dtype=th.float32).reshape(1, 96, 1, 1).to(self.device)
        std = th.as_tensor(np.asarray(stds), dtype=th.float32).reshape(1, 96, 1, 1).to(self.device)
        init = th.randn((1, 96, S, S), generator=gen, device=self.device) * std + mean
        planes, self.last_losses = fit_triplanes(self.decoder, points, occupancies, init, epochs=epochs,
                                                 batch_size=batch_size, lr=lr, generator=gen, batch_fn=batch_fn)
        fitted = planes_to_latent(planes)
        self.decoder.embeddings = [fitted[:, 32 * i:32 * (i + 1)].clone() for i in range(3)]
        latent = (fitted - self.middle) / self.range
        np.save(os.path.join(path, "tri_feat_opt.npy"), latent.cpu().numpy())
        mesh_backend.write_mesh(os.path.join(path, "mesh_opt.obj"), self.get_mesh(latent))
        return latent

    def latent_inversion(self, tri_feat, fwd_noise=None):
        """DDPM inversion of `tri_feat` to the edit's start latent (self.w) and guidance taps.  Every step runs its forward; the
        new self.w invalidates the first-step snapshot of training()."""
        self._shape_changed()
        outs = self.diffusion.ddpm_inversion(self.model, tri_feat, self.args.w_time, fwd_noise=fwd_noise,
                                             clip_denoised=self.args.clip_denoised, feat_layer=self.args.feat_layer,
                                             want_inter_feat=False, tap_sink=self._tap_sink_reset())
        self.w = outs["latent"].clone().detach()
        self.w0 = self.w.clone().detach()
        self.feature_guidance = list(self._sink)
        self.mesh = self.get_mesh(tri_feat=outs["sample"])
        self.mesh0 = copy.deepcopy(self.mesh)
        self.tri_feat0 = outs["sample"].detach().to(self.device).clone()
        self.variance = [v.clone().detach() for v in outs["variance"]]
        self.variance_noise = [v.clone().detach() for v in outs["variance_noise"]]

    def _tap_sink_reset(self):
        self._sink = []
        return lambda: self._sink.append(self.model.copy_tap(self.args.feat_layer)[0])

    def clear_params(self):
        self._shape_changed()
        self.mesh0 = None
        self.tri_feat0 = None
        self.mesh = None
        self.latent_code = None
        self.w0 = None
        self.w = None
        self.feature_guidance.clear()
        self.noise.clear()
        self.variance.clear()
        self.variance_noise.clear()

    def reset_params(self):
        if self.mesh is not None:
            self.mesh = copy.deepcopy(self.mesh0)
        if self.w0 is not None:
            self.w = self.w0.clone().detach()
