"""Host-side mirror of guided_diffusion/unet.py:UNetModel backed by libishap_hip.so.

Same call surface as the reference module for the path the editor uses
(`model(x, timesteps, feat_layer=k)` -> `(out, inter_feat)` or `out`, `load_state_dict(strict=True)`,
`convert_to_fp16()`, `eval()`, `parameters()`), but the network itself is one C call that
enqueues the hand-written HIP kernels on torch's current stream.  torch only owns the tensors.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from . import _lib
from .unet_spec import UNetConfig, build_spec, param_shapes


class UNetModel:
    def __init__(self, cfg: UNetConfig, device: Optional[torch.device] = None, max_batch: int = 1):
        if not cfg.use_fp16:
            raise NotImplementedError("the path's precision contract is use_fp16=True (drag_utils.py:51, "
                                      "generate.py:67): fp16 torso, fp32 norms/embeddings/head")
        self.cfg = cfg
        self.spec = build_spec(cfg)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("UNetModel needs a GPU device: there is no CPU fallback")
        self.image_size = cfg.image_size
        self.in_channels = cfg.in_channels
        self.out_channels = cfg.out_channels
        self.model_channels = cfg.model_channels
        self.dtype = torch.float16
        self.max_batch = max_batch
        self._L = _lib.lib()
        c = _lib.UNetConfigC()
        c.image_size, c.in_channels, c.model_channels = cfg.image_size, cfg.in_channels, cfg.model_channels
        c.out_channels, c.num_res_blocks = cfg.out_channels, cfg.num_res_blocks
        mult = cfg.resolved_channel_mult()
        if any(int(m) != m for m in mult):
            raise NotImplementedError("fractional channel_mult (image_size 512) is not on the path")
        c.n_mult = len(mult)
        for i, m in enumerate(mult):
            c.channel_mult[i] = int(m)
        att = cfg.attention_ds()
        c.n_att = len(att)
        for i, a in enumerate(att):
            c.attention_ds[i] = int(a)
        c.num_head_channels = cfg.num_head_channels
        c.max_batch = max_batch
        h = C.c_void_p()
        _lib.call(self.device, "ishap_unet_create", C.byref(c), self.device.index or 0, C.byref(h), stream=False)
        self._h = h
        self._param_probe = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._fp16 = False
        self._last_shape, self._last_feat = None, -1
        self._last_cot = None
        self._snap_key = None          # (N, feat_layer, input shape) of the forward a valid snapshot holds

    def _call(self, name: str, *args, stream=True):
        """the library entry `name` on this context: _lib.call with the handle as first argument"""
        _lib.call(self.device, name, self._h, *args, stream=stream)

    # ------------------------------------------------------------------ module-like surface
    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.ishap_unet_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def to(self, device):
        if torch.device(device).type != "cuda":
            raise RuntimeError("UNetModel lives on the GPU it was created on")
        return self

    def eval(self):
        return self

    def parameters(self) -> Iterator[torch.Tensor]:
        # drag_utils.py:257-264 only asks the first parameter for its dtype (time_embed.0.weight: fp32)
        yield self._param_probe

    def convert_to_fp16(self):
        """unet.py:618-624 -- the packed weights already follow that contract (done at load)."""
        self._fp16 = True
        self.snapshot_drop()

    def param_table(self) -> Dict[str, tuple]:
        out = {}
        name = C.create_string_buffer(256)
        nd = C.c_int()
        shp = (C.c_longlong * 4)()
        for i in range(self._L.ishap_unet_num_params(self._h)):
            self._call("ishap_unet_param_info", i, name, 256, C.byref(nd), shp, stream=False)
            out[name.value.decode()] = tuple(int(shp[k]) for k in range(nd.value))
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        table = param_shapes(self.cfg)
        missing = [k for k in table if k not in sd]
        unexpected = [k for k in sd if k not in table]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing keys {missing[:5]}..., "
                               f"unexpected keys {unexpected[:5]}...")
        s = _lib.stream_ptr(self.device)
        self._snap_key = None          # the library drops the snapshot's validity with the first tensor it loads
        for k, shape in table.items():
            if k not in sd:
                continue
            v = sd[k]
            if tuple(v.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)} vs {tuple(shape)}")
            v = _lib.tensor(v, torch.float32, self.device)
            self._call("ishap_unet_load_param", k.encode(), v.data_ptr(), v.numel(), stream=s)     # the stream fetched once
            del v
        torch.cuda.current_stream(self.device).synchronize()
        return self

    # ------------------------------------------------------------------ forward / backward
    def forward(self, x: torch.Tensor, timesteps, y=None, feat_layer: int = -1, keep_for_backward: bool = False,
                want_inter_feat: bool = True, overlap_tail: bool = False):
        """`overlap_tail` (with a tap): the blocks after the tap and the head are only PLANNED; `run_tail()` enqueues them on the
        context's own stream beside whatever the caller has enqueued meanwhile (loss, backward) -- a join, the next forward or a
        full-depth backward does so by itself.  The returned model output is valid only after `join_tail()`; the model keeps a
        reference to it until then (the library writes it through the raw pointer)."""
        assert y is None, "class conditioning is not on the path"
        assert x.dim() == 4 and x.shape[1] == self.in_channels and x.shape[2] == x.shape[3] == self.image_size
        N = x.shape[0]
        x = _lib.tensor(x, torch.float32, self.device)
        ts = (C.c_float * N)(*[float(t) for t in (timesteps.tolist() if torch.is_tensor(timesteps) else timesteps)])
        out = torch.empty((N, self.out_channels, self.image_size, self.image_size), dtype=torch.float32,
                          device=self.device)
        inter = None
        if feat_layer >= 0 and want_inter_feat:
            ch, sz = C.c_int(), C.c_int()
            self._call("ishap_unet_tap_shape", feat_layer, C.byref(ch), C.byref(sz), stream=False)
            inter = torch.empty((N, ch.value, sz.value, sz.value), dtype=torch.float16, device=self.device)
        self._call("ishap_unet_forward", x.data_ptr(), ts, N, int(feat_layer), out.data_ptr(), _lib.ptr(inter),
                   int(bool(keep_for_backward)) | (2 if overlap_tail else 0))
        self._last_shape, self._last_feat = tuple(x.shape), int(feat_layer)
        if self._snap_key is not None and self._snap_key[:2] != (N, int(feat_layer)):
            self._snap_key = None      # the library invalidates a snapshot when a forward has another batch size or tap
        self._tail_out = out if overlap_tail else None       # alive until the tail that writes it has been joined
        if feat_layer < 0:
            return out
        return out, inter

    __call__ = forward

    def run_tail(self):
        """Enqueue the forward tail that `forward(overlap_tail=True)` only planned; no-op when there is none."""
        self._call("ishap_unet_run_tail", stream=False)

    def join_tail(self):
        """Order the current stream behind an overlapped forward tail (no-op when there is none)."""
        self._call("ishap_unet_join_tail")
        self._tail_out = None

    # ------------------------------------------------------------------ snapshot of a kept forward
    def snapshot_save(self) -> bool:
        """Copy what `backward_input` reads of the last forward(keep_for_backward=True) -- saved activations up to the tap,
        statistics, FiLM rows, the tap -- into buffers the context keeps; joins a pending tail first.  False: unavailable
        (the per-launch profile is recording), nothing was saved."""
        with torch.cuda.device(self.device):
            rc = self._L.ishap_unet_snapshot_save(self._h, _lib.stream_ptr(self.device))
        if rc == 1:
            return False
        _lib.check(rc)
        self._tail_out = None
        self._snap_key = (self._last_shape[0], self._last_feat, self._last_shape)
        return True

    def snapshot_restore(self) -> bool:
        """Put the snapshot back: afterwards `tap_ptr`, `copy_tap` and `backward_input` behave as after the forward it was taken
        of (a full-depth backward does not, when that forward planned a tail).  False: unavailable (the per-launch profile is
        recording) -- run the forward instead.  Raises when there is no valid snapshot."""
        with torch.cuda.device(self.device):
            rc = self._L.ishap_unet_snapshot_restore(self._h, _lib.stream_ptr(self.device))
        if rc == 1:
            return False
        _lib.check(rc)
        self._tail_out = None
        if self._snap_key is not None:
            self._last_shape, self._last_feat = self._snap_key[2], self._snap_key[1]
        return True

    def has_snapshot(self) -> bool:
        """A snapshot was saved and nothing has invalidated it since (weight load, convert_to_fp16, a forward of another batch
        size or tap)."""
        return self._snap_key is not None

    def snapshot_drop(self):
        self._snap_key = None
        if getattr(self, "_h", None):
            self._call("ishap_unet_snapshot_drop", stream=False)

    def snapshot_bytes(self) -> int:
        return int(self._L.ishap_unet_snapshot_bytes(self._h))

    def prepare_timesteps(self, timesteps):
        """Compute the timestep-dependent FiLM rows of a sampling loop once (they do not depend on x): forwards at these
        timesteps skip the embedding launches.  An empty list drops them.  Values are bit-identical either way."""
        ts = [float(t) for t in timesteps]
        arr = (C.c_float * max(len(ts), 1))(*ts)
        self._call("ishap_unet_prepare_timesteps", arr, len(ts))

    def tap_shape(self, feat_layer: int):
        ch, sz = C.c_int(), C.c_int()
        self._call("ishap_unet_tap_shape", feat_layer, C.byref(ch), C.byref(sz), stream=False)
        return ch.value, sz.value

    def tap_ptr(self) -> int:
        return self._L.ishap_unet_tap_ptr(self._h)

    def copy_tap(self, feat_layer: int, N: Optional[int] = None) -> torch.Tensor:
        """The resident tap of the last forward as an NHWC fp16 tensor [N, S*S, C] (device copy); N is the last forward's
        batch size (the library copies that many images)."""
        ch, sz = self.tap_shape(feat_layer)
        last = self._last_shape[0] if self._last_shape is not None else 1
        if N is not None and N != last:
            raise ValueError(f"copy_tap: the resident tap holds {last} image(s), not {N}")
        N = last
        t = torch.empty((N, sz * sz, ch), dtype=torch.float16, device=self.device)
        self._call("ishap_unet_copy_tap", t.data_ptr())
        return t

    def block_output(self, group: int, index: int = 0) -> torch.Tensor:
        """Output of input_blocks[index] (group 0), middle_block (1) or output_blocks[index] (2) of the last
        forward(keep_for_backward=True), as fp16 NCHW like the reference's activations.  The batch size is the kept
        forward's (the library writes that many images)."""
        ch, sz = C.c_int(), C.c_int()
        self._call("ishap_unet_block_output", group, index, C.byref(ch), C.byref(sz), None, None, stream=False)
        if self._last_shape is None:
            raise RuntimeError("block outputs stay resident only after a forward with keep_for_backward=1")
        t = torch.empty((self._last_shape[0], ch.value, sz.value, sz.value), dtype=torch.float16, device=self.device)
        self._call("ishap_unet_block_output", group, index, C.byref(ch), C.byref(sz), t.data_ptr())
        return t

    def block_grad(self, group: int, index: int = 0, part: int = 0) -> torch.Tensor:
        """A gradient map of the last `backward_input` / `backward_from_output`, as fp16 NCHW, exactly as stored (a loss scale
        stays in it): part 0 = the gradient w.r.t. the output of input_blocks[index] (group 0), middle_block (1) or
        output_blocks[index] (2), summed over all its consumers; parts 1 / 2 (group 2 only) = the gradient w.r.t. the `h` / the
        `skip` half of the output block's concatenated input.  The maps stay resident until the next forward, backward or
        snapshot restore; a read after one of those raises."""
        ch, sz = C.c_int(), C.c_int()
        self._call("ishap_unet_block_grad", group, index, part, C.byref(ch), C.byref(sz), None, None, stream=False)
        if self._last_shape is None:
            raise RuntimeError("block gradients exist only after a backward pass on this context")
        t = torch.empty((self._last_shape[0], ch.value, sz.value, sz.value), dtype=torch.float16, device=self.device)
        self._call("ishap_unet_block_grad", group, index, part, C.byref(ch), C.byref(sz), t.data_ptr())
        return t

    def workspace_bytes(self) -> int:
        return int(self._L.ishap_unet_workspace_bytes(self._h))

    def backward_input(self, cot_nhwc_f16: torch.Tensor, scale2: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Gradient w.r.t. x of sum(tap * cot) for the last forward(keep_for_backward=True)."""
        dx = torch.empty(self._last_shape, dtype=torch.float32, device=self.device)
        self._call("ishap_unet_backward_input", cot_nhwc_f16.data_ptr(), _lib.ptr(scale2), dx.data_ptr())
        self._last_cot = cot_nhwc_f16      # block_grad reads the tapped block's incoming gradient through this buffer
        return dx

    def backward_from_output(self, cot_out: torch.Tensor, scale2: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Full-depth input gradient of sum(out * cot).  `cot_out` fp32, or fp16 pre-multiplied by scale2[0]."""
        dx = torch.empty(self._last_shape, dtype=torch.float32, device=self.device)
        is_f16 = cot_out.dtype == torch.float16
        cot_out = _lib.tensor(cot_out, None, self.device)
        if not is_f16:
            cot_out = cot_out.float()
        self._call("ishap_unet_backward_from_output", cot_out.data_ptr(), int(is_f16), _lib.ptr(scale2), dx.data_ptr())
        return dx
