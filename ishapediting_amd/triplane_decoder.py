"""Host-side mirror of triplane_decoder/axisnetworks.py:MultiTriplane and the dense-grid decode of
triplane_decoder/visualize.py:create_obj_o3d, backed by the fp32-MFMA decode kernel.

`decoder.net.load_state_dict(...)`, `decoder.embeddings[i] = plane[1,32,S,S]` and
`decoder(obj_idx, coords[1,N,3]) -> logits[1,N,1]` work as in the reference
(drag_utils.py:188,246,295-298,455).  The grid decode keeps the whole 256^3 volume on the device
instead of 336 host round trips (visualize.py:89-95).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional

import torch

from . import _lib
from .unet_spec import DECODER_SHAPES

# train_triplane_opt's loss weights and optimiser (drag_utils.py:516-539)
PAIR_WEIGHT, L2_WEIGHT, TV_WEIGHT = 0.3, 0.001, 0.01
REG_WS = 576          # doubles of regulariser workspace (ISHAP_TRIPLANE_REG_WS, include/ishap.h)
PROJECT_GMIN = 1e-12  # |d logit / d coordinate|^2 below which a point has no usable direction (project_to_surface)
DECODE_RES = 256      # the decoding grid project_to_surface's default step lengths are voxels of (visualize.py:79-81)


class FieldGrad(NamedTuple):
    """field_grad_planes: logits [N] and d logit / d coordinate [N,3]"""
    logits: torch.Tensor
    grad: torch.Tensor


class Projection(NamedTuple):
    """project_to_surface: the moved points [N,3], their logits [N], unit normals [N,3] (outward; 0 where the gradient
    vanishes) and the number of accepted steps [N] int32"""
    points: torch.Tensor
    logits: torch.Tensor
    normals: torch.Tensor
    accepted: torch.Tensor


class ConstraintState(NamedTuple):
    """MultiTriplane.constraint_setup: the points of an edit's volume constraints (coords [M,3], targets [M], weights [M], the
    weights' sum as a Python float), the gather list of their taps on planes of side S (row_start int32 [3 S S + 1], entry int32
    and entry_w float32 [12 M], the first row_start[-1] used) and the per-step scratch (dfeat [M,32], partials [ceil(M / 32)])"""
    coords: torch.Tensor
    targets: torch.Tensor
    weights: torch.Tensor
    wsum: float
    S: int
    row_start: torch.Tensor
    entry: torch.Tensor
    entry_w: torch.Tensor
    dfeat: torch.Tensor
    partials: torch.Tensor

    @property
    def M(self) -> int:
        return int(self.coords.shape[0])


class _Net:
    """Stands in for the nn.Sequential `net` (axisnetworks.py:526-535): holds the seven tensors on the device."""

    def __init__(self, device):
        self.device = device
        self.sd: Dict[str, torch.Tensor] = {k: torch.zeros(s, dtype=torch.float32, device=device)
                                            for k, s in DECODER_SHAPES.items()}
        self.loaded = False

    def load_state_dict(self, sd, strict: bool = True):
        missing = [k for k in DECODER_SHAPES if k not in sd]
        unexpected = [k for k in sd if k not in DECODER_SHAPES]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing}, unexpected {unexpected}")
        for k, shape in DECODER_SHAPES.items():
            if k in sd:
                v = sd[k]
                if tuple(v.shape) != tuple(shape):
                    raise RuntimeError(f"size mismatch for {k}")
                self.sd[k] = _lib.tensor(v, torch.float32, self.device)
        self.loaded = True

    def state_dict(self):
        return dict(self.sd)

    def parameters(self):
        return iter(self.sd.values())

    def weights_c(self) -> _lib.DecoderWeightsC:
        s = self.sd
        return _lib.DecoderWeightsC(s["0._B"].data_ptr(), s["1.weight"].data_ptr(), s["1.bias"].data_ptr(),
                                    s["3.weight"].data_ptr(), s["3.bias"].data_ptr(), s["5.weight"].data_ptr(),
                                    s["5.bias"].data_ptr())


class MultiTriplane:
    def __init__(self, num_objs: int = 1, input_dim: int = 3, output_dim: int = 1, noise_val=None, device="cuda"):
        assert input_dim == 3 and output_dim == 1
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MultiTriplane needs a GPU device: there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_objs = num_objs
        self.embeddings: List[torch.Tensor] = [torch.randn(1, 32, 128, 128, device=self.device) * 0.001
                                               for _ in range(3 * num_objs)]
        self.net = _Net(self.device)
        self.training = False

    def to(self, device):
        return self

    def eval(self):
        self.training = False
        return self

    def _planes(self, obj_idx: int) -> torch.Tensor:
        """embeddings[3*obj..] ([1,32,S,S] each) -> channels-last [3][S][S][32] for the kernel."""
        e = [self.embeddings[3 * obj_idx + i] for i in range(3)]
        S = e[0].shape[-1]
        latent = torch.cat([t.reshape(1, 32, S, S) for t in e], dim=1).to(device=self.device, dtype=torch.float32).contiguous()
        planes = torch.empty((3, S, S, 32), dtype=torch.float32, device=self.device)
        _lib.call(self.device, "ishap_planes_prepare", latent.data_ptr(), None, None, S, planes.data_ptr())
        return planes

    def forward(self, obj_idx: int, coordinates: torch.Tensor, debug: bool = False) -> torch.Tensor:
        """axisnetworks.py:546-562: coordinates [B, N, 3] -> logits [B, N, 1]."""
        b, n, d = coordinates.shape
        assert d == 3
        planes = self._planes(obj_idx)
        coords = _lib.tensor(coordinates, torch.float32, self.device, (-1, 3))
        out = torch.empty(coords.shape[0], dtype=torch.float32, device=self.device)
        w = self.net.weights_c()
        _lib.call(self.device, "ishap_triplane_decode_points", planes.data_ptr(), planes.shape[1], C.byref(w), coords.data_ptr(),
                  coords.shape[0], out.data_ptr())
        return out.reshape(b, n, 1)

    __call__ = forward

    def field_grad(self, obj_idx: int, coordinates: torch.Tensor):
        """The forward's logits together with their derivative in space: coordinates [B, N, 3] ->
        (logits [B, N, 1], grad [B, N, 3] = d logit / d coordinate), see field_grad_planes."""
        b, n, d = coordinates.shape
        assert d == 3
        r = field_grad_planes(self, self._planes(obj_idx), coordinates)
        return r.logits.reshape(b, n, 1), r.grad.reshape(b, n, 3)

    def points_loss_grad(self, planes: torch.Tensor, coords: torch.Tensor, gt: torch.Tensor):
        """drag_utils.py:455-458 on explicit planes: loss = -BCEWithLogitsLoss()(decoder(coords), gt) and
        d loss / d planes ([3,S,S,32]); also returns the logits."""
        coords = _lib.tensor(coords, torch.float32, self.device, (-1, 3))
        gt = _lib.tensor(gt, torch.float32, self.device, (-1,))
        assert coords.shape[0] == gt.shape[0]
        sd = self.net.sd
        w1t, w2t = sd["1.weight"].t().contiguous(), sd["3.weight"].t().contiguous()
        dplanes = torch.empty_like(planes)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        logits = torch.empty(coords.shape[0], dtype=torch.float32, device=self.device)
        w = self.net.weights_c()
        _lib.call(self.device, "ishap_triplane_points_loss_grad",
                  planes.data_ptr(), planes.shape[1], C.byref(w), w1t.data_ptr(), w2t.data_ptr(), coords.data_ptr(),
                  gt.data_ptr(), coords.shape[0], dplanes.data_ptr(), loss.data_ptr(), logits.data_ptr())
        return loss, dplanes, logits

    def constraint_setup(self, coords: torch.Tensor, targets: torch.Tensor, weights: torch.Tensor, S: int) -> "ConstraintState":
        """Once per edit (ishap_constraint_setup): the gather list of the 12 bilinear taps of every constraint point on planes
        of side S, and the buffers constraint_loss_grad works in.  coords [M, 3], targets [M] in {0, 1}, weights [M] >= 0 with a
        positive sum (summed here in double: the one host read)."""
        dev = self.device
        f32 = dict(device=dev, dtype=torch.float32)
        coords = _lib.tensor(coords, torch.float32, dev, (-1, 3))
        targets = _lib.tensor(targets, torch.float32, dev, (-1,))
        weights = _lib.tensor(weights, torch.float32, dev, (-1,))
        M, S = coords.shape[0], int(S)
        if targets.shape[0] != M or weights.shape[0] != M:
            raise ValueError(f"constraint_setup: {M} points, {targets.shape[0]} targets, {weights.shape[0]} weights")
        try:
            scratch, nbytes = _lib.scratch(dev, "ishap_constraint_setup_scratch_bytes", M, S)
        except _lib.ScratchError:
            raise ValueError(f"constraint_setup: M = {M}, S = {S} is outside 1 <= M <= 2^20, 2 <= S <= 1024") from None
        if not bool(torch.isfinite(weights).all()) or bool((weights < 0).any()):
            raise ValueError("constraint_setup: weights must be finite and >= 0")
        wsum = float(weights.double().sum())
        if not wsum > 0:
            raise ValueError("constraint_setup: the weights must have a positive sum")
        row_start = torch.empty(3 * S * S + 1, dtype=torch.int32, device=dev)
        entry = torch.empty(12 * M, dtype=torch.int32, device=dev)
        entry_w = torch.empty(12 * M, **f32)
        _lib.call(dev, "ishap_constraint_setup", coords.data_ptr(), M, S, row_start.data_ptr(), entry.data_ptr(), entry_w.data_ptr(),
                  scratch.data_ptr(), nbytes)
        return ConstraintState(coords, targets, weights, wsum, S, row_start, entry, entry_w,
                               torch.empty((M, 32), **f32), torch.empty((M + 31) // 32, **f32))

    def constraint_loss_grad(self, planes: torch.Tensor, state: "ConstraintState", dplanes: Optional[torch.Tensor] = None,
                             loss: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None):
        """L_vol = -(1 / sum w) sum_j w_j BCEWithLogits(decoder(planes)(q_j), g_j) at the points of `state` and d L_vol / d planes
        ([3,S,S,32], every texel written) -> (loss [1], dplanes, logits or None).  dplanes / loss are allocated when None;
        logits [M] are written only into a tensor given here.  Two launches, no float atomics: bitwise repeatable."""
        dev = self.device
        assert planes.dtype == torch.float32 and planes.is_contiguous() and tuple(planes.shape) == (3, state.S, state.S, 32)
        if dplanes is None:
            dplanes = torch.empty_like(planes)
        if loss is None:
            loss = torch.empty(1, dtype=torch.float32, device=dev)
        assert dplanes.is_contiguous() and dplanes.shape == planes.shape and dplanes.dtype == torch.float32
        assert logits is None or (logits.dtype == torch.float32 and logits.numel() == state.M and logits.is_contiguous())
        w = self.net.weights_c()
        _lib.call(dev, "ishap_constraint_loss_grad",
                  planes.data_ptr(), state.S, C.byref(w), state.coords.data_ptr(), state.targets.data_ptr(), state.weights.data_ptr(),
                  state.M, state.wsum, state.row_start.data_ptr(), state.entry.data_ptr(), state.entry_w.data_ptr(),
                  state.dfeat.data_ptr(), state.partials.data_ptr(), dplanes.data_ptr(), loss.data_ptr(), _lib.ptr(logits))
        return loss, dplanes, logits

    def fit_loss_grad(self, planes: torch.Tensor, coords: torch.Tensor, gt: torch.Tensor, idx: torch.Tensor,
                      rand_coords: torch.Tensor, rand_noise: torch.Tensor, dplanes: Optional[torch.Tensor] = None,
                      loss_parts: Optional[torch.Tensor] = None, pair_weight: float = PAIR_WEIGHT):
        """The decoder terms of one train_triplane_opt step (drag_utils.py:526-535) on explicit channels-last planes
        [3,S,S,32]: BCEWithLogits(decoder(coords[idx]), gt[idx]) + pair_weight * mse(decoder(r), decoder(r + 0.01 * noise)).
        Adds d loss / d planes into `dplanes` and {BCE, mse} into `loss_parts` (both zero-allocated when None, both device
        tensors) and returns (loss_parts, dplanes).  One kernel launch, no host synchronisation."""
        dev = self.device
        f32 = dict(device=dev, dtype=torch.float32)
        coords = _lib.tensor(coords, torch.float32, dev, (-1, 3))
        gt = _lib.tensor(gt, torch.float32, dev, (-1,))
        idx = _lib.tensor(idx, torch.int32, dev, (-1,))
        rc = _lib.tensor(rand_coords, torch.float32, dev, (-1, 3))
        rn = _lib.tensor(rand_noise, torch.float32, dev, (-1, 3))
        assert coords.shape[0] == gt.shape[0] and rc.shape == rn.shape
        assert planes.dtype == torch.float32 and planes.is_contiguous() and planes.shape[0] == 3 and planes.shape[3] == 32
        if dplanes is None:
            dplanes = torch.zeros_like(planes)
        if loss_parts is None:
            loss_parts = torch.zeros(2, **f32)
        w = self.net.weights_c()
        _lib.call(dev, "ishap_triplane_fit_loss_grad",
                  planes.data_ptr(), planes.shape[1], C.byref(w), coords.data_ptr(), gt.data_ptr(), idx.data_ptr(), idx.numel(),
                  rc.data_ptr(), rn.data_ptr(), rc.shape[0], float(pair_weight), dplanes.data_ptr(), loss_parts.data_ptr())
        return loss_parts, dplanes

    def _reg_values(self) -> torch.Tensor:
        """{l2reg, tvreg} summed over the objects' planes, divided by num_objs (axisnetworks.py:564-575)."""
        out = torch.zeros(2, dtype=torch.float32, device=self.device)
        for o in range(self.num_objs):
            out += reg_values(self._planes(o))
        return out / self.num_objs

    def l2reg(self) -> torch.Tensor:
        """axisnetworks.py:571-575: sum of the planes' L2 norms / num_objs, as a device scalar."""
        return self._reg_values()[0]

    def tvreg(self) -> torch.Tensor:
        """axisnetworks.py:564-569: sum of the planes' H and W total-variation norms / num_objs, as a device scalar."""
        return self._reg_values()[1]


def prepare_planes(latent: torch.Tensor, rng: Optional[torch.Tensor], mid: Optional[torch.Tensor]) -> torch.Tensor:
    """(tri_feat * range + middle).reshape(3,32,S,S) (drag_utils.py:295) as channels-last planes, one kernel."""
    assert latent.shape[0] == 1 and latent.shape[1] == 96
    dev = latent.device
    S = latent.shape[-1]
    latent = _lib.tensor(latent, torch.float32)

    def vec(v, default):
        if v is None:
            return None
        if torch.is_tensor(v):
            v = v.detach().to(device=dev, dtype=torch.float32).reshape(-1)
            return (v.expand(96) if v.numel() == 1 else v).contiguous()
        return None if float(v) == default else torch.full((96,), float(v), dtype=torch.float32, device=dev)
    r, m = vec(rng, 1.0), vec(mid, 0.0)
    planes = torch.empty((3, S, S, 32), dtype=torch.float32, device=dev)
    _lib.call(dev, "ishap_planes_prepare", latent.data_ptr(), _lib.ptr(r), _lib.ptr(m), S, planes.data_ptr())
    return planes


def decode_planes_grid(decoder: MultiTriplane, planes: torch.Tensor, res: int) -> torch.Tensor:
    """visualize.py:79-97: occupancy logits on linspace(-1,1,res)^3 ('ij', x slowest) -> [res,res,res] on device."""
    dev = planes.device
    axis = torch.linspace(-1, 1, res).to(dev)          # same values the reference builds on the host (:79-81)
    vol = torch.empty((res, res, res), dtype=torch.float32, device=dev)
    w = decoder.net.weights_c()
    _lib.call(dev, "ishap_triplane_decode_grid", planes.data_ptr(), planes.shape[1], C.byref(w), axis.data_ptr(), res, vol.data_ptr())
    return vol


def decode_bricks(decoder: MultiTriplane, planes: torch.Tensor, res: int, bricks: torch.Tensor) -> torch.Tensor:
    """Occupancy logits on the 9^3 sample nodes of `bricks` (int [n] ids (bx nb + by) nb + bz, nb = ceil((res - 1) / 8)) of the
    fine grid linspace(-1, 1, res)^3 -> [n,9,9,9] on the device: brick b samples nodes 8 b .. 8 b + 8 per axis, indices above
    res - 1 clamped.  Bit for bit decode_planes_grid(decoder, planes, res) at those nodes, without the res^3 volume
    (ishap_triplane_decode_bricks; mesh.extract_surface_sparse is its user)."""
    dev = planes.device
    res = int(res)
    ids = _lib.tensor(bricks, torch.int32, dev, (-1,))
    n = int(ids.shape[0])
    nb = int(_lib.lib().ishap_sparse_bricks_per_axis(res))
    if nb < 0:
        raise ValueError(f"decode_bricks: res = {res} is outside 9 .. 2048")
    if n == 0:
        return torch.empty((0, 9, 9, 9), dtype=torch.float32, device=dev)
    if int(ids.min()) < 0 or int(ids.max()) >= nb ** 3:
        raise ValueError(f"decode_bricks: brick ids must lie in 0 .. {nb ** 3 - 1} (res = {res}: {nb} bricks per axis)")
    out = torch.empty((n, 9, 9, 9), dtype=torch.float32, device=dev)
    _decode_bricks_into(decoder, planes, torch.linspace(-1, 1, res).to(dev), res, ids, out)
    return out


def _decode_bricks_into(decoder: MultiTriplane, planes: torch.Tensor, axis: torch.Tensor, res: int, ids: torch.Tensor, out: torch.Tensor):
    """ishap_triplane_decode_bricks on checked arguments: ids int32 [n] (n >= 1) -> out float32 [n,9,9,9], both contiguous"""
    w = decoder.net.weights_c()
    _lib.call(planes.device, "ishap_triplane_decode_bricks", planes.data_ptr(), planes.shape[1], C.byref(w), axis.data_ptr(), res,
              ids.data_ptr(), ids.shape[0], out.data_ptr())


def decode_volume(decoder: MultiTriplane, latent: torch.Tensor, rng, mid, res: int) -> torch.Tensor:
    """get_mesh's decode half (drag_utils.py:295-298 + visualize.py:79-97) without leaving the device."""
    return decode_planes_grid(decoder, prepare_planes(latent, rng, mid), res)


def _field_inputs(decoder: MultiTriplane, planes: torch.Tensor, coords: torch.Tensor):
    assert planes.dtype == torch.float32 and planes.is_contiguous() and planes.dim() == 4 and planes.shape[0] == 3 and planes.shape[3] == 32
    c = _lib.tensor(coords, torch.float32, planes.device, (-1, 3))
    if c.shape[0] == 0:
        raise ValueError("the decoder's field needs at least one point")
    return c, decoder.net.weights_c()


def field_grad_planes(decoder: MultiTriplane, planes: torch.Tensor, coords: torch.Tensor) -> FieldGrad:
    """MultiTriplane.forward (axisnetworks.py:537-562) on explicit channels-last planes [3,S,S,32] with its analytic
    derivative in space: coords [..., 3] -> FieldGrad(logits [N], grad [N,3]).  On a cell boundary of a plane the
    derivative is the right-sided one; outside every plane it is exactly 0.  One launch, bitwise repeatable."""
    dev = planes.device
    c, w = _field_inputs(decoder, planes, coords)
    logits = torch.empty(c.shape[0], dtype=torch.float32, device=dev)
    grad = torch.empty((c.shape[0], 3), dtype=torch.float32, device=dev)
    _lib.call(dev, "ishap_triplane_field_grad", planes.data_ptr(), planes.shape[1], C.byref(w), c.data_ptr(), c.shape[0],
              logits.data_ptr(), grad.data_ptr())
    return FieldGrad(logits, grad)


def project_to_surface(decoder: MultiTriplane, planes: torch.Tensor, coords: torch.Tensor, iterations: int = 4,
                       step_max: float = 0.5 * 2.0 / (DECODE_RES - 1), max_move: float = 1.0 * 2.0 / (DECODE_RES - 1),
                       tol: float = 1e-4, gmin: float = PROJECT_GMIN) -> Projection:
    """Move coords [..., 3] onto the zero level set of the decoder's field by `iterations` damped Newton steps along the
    gradient (ishap_triplane_project): a step is taken only when it lowers |logit|, no single step is longer than `step_max`
    and no point ends further than `max_move` from where it started -- by default 0.5 and 1.0 voxels of the 256^3
    decoding grid, in decoder coordinates.  Points with |logit| <= tol are left alone.  The normals are -grad / |grad|, the
    direction of decreasing logit: logits are positive inside (level 0, extract_surface), so they point OUTWARD.
    iterations = 0: the logit and the normal at the given points."""
    dev = planes.device
    c, w = _field_inputs(decoder, planes, coords)
    n = c.shape[0]
    out = Projection(torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                     torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    _lib.call(dev, "ishap_triplane_project", planes.data_ptr(), planes.shape[1], C.byref(w), c.data_ptr(), n, int(iterations),
              float(step_max), float(max_move), float(tol), float(gmin), out.points.data_ptr(), out.logits.data_ptr(),
              out.normals.data_ptr(), out.accepted.data_ptr())
    return out


def reg_values(planes: torch.Tensor) -> torch.Tensor:
    """{l2reg, tvreg} (axisnetworks.py:564-575, one object) of channels-last planes [3,S,S,32] as a device float[2]."""
    dev = planes.device
    out = torch.empty(2, dtype=torch.float32, device=dev)
    ws = torch.empty(REG_WS, dtype=torch.float64, device=dev)
    planes = _lib.tensor(planes, torch.float32)
    _lib.call(dev, "ishap_triplane_reg_values", planes.data_ptr(), planes.shape[1], ws.data_ptr(), out.data_ptr())
    return out


class TriplaneAdam:
    """torch.optim.Adam(planes, lr, betas, eps) for channels-last planes [3,S,S,32], with train_triplane_opt's two
    regularisers folded into the step (drag_utils.py:536-539).  m, v and the step count live on the device; `step()` reads
    the accumulated `dplanes`, adds the regulariser gradients, steps and leaves `dplanes` zeroed.  The planes alternate
    between two buffers: `planes` is the current one."""

    def __init__(self, planes: torch.Tensor, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 l2_weight: float = L2_WEIGHT, tv_weight: float = TV_WEIGHT):
        assert planes.dtype == torch.float32 and planes.dim() == 4 and planes.shape[0] == 3 and planes.shape[3] == 32
        self.planes = planes.detach().clone().contiguous()
        self._spare = torch.empty_like(self.planes)
        self.m = torch.zeros_like(self.planes)
        self.v = torch.zeros_like(self.planes)
        self.dplanes = torch.zeros_like(self.planes)
        self.step_count = torch.zeros(1, dtype=torch.int32, device=planes.device)
        self.ws = torch.empty(REG_WS, dtype=torch.float64, device=planes.device)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.l2_weight, self.tv_weight = float(l2_weight), float(tv_weight)

    def step(self, reg_parts: Optional[torch.Tensor] = None):
        """One Adam step; `reg_parts` (device float[2] or None) receives {l2reg, tvreg} of the planes before the step."""
        _lib.call(self.planes.device, "ishap_triplane_reg_adam_step",
                  self.planes.data_ptr(), self._spare.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.dplanes.data_ptr(),
                  self.planes.shape[1], self.step_count.data_ptr(), self.lr, self.betas[0], self.betas[1], self.eps,
                  self.l2_weight, self.tv_weight, self.ws.data_ptr(), _lib.ptr(reg_parts))
        self.planes, self._spare = self._spare, self.planes
        return self.planes


def batch_schedule(n: int, batch_size: int):
    """DataLoader(batch_size, shuffle=True)'s batches over n samples: (start, count) into the epoch's permutation,
    the last one partial when batch_size does not divide n."""
    if n <= 0 or batch_size <= 0:
        raise ValueError(f"need points and a positive batch size (n={n}, batch_size={batch_size})")
    return [(s, min(batch_size, n - s)) for s in range(0, n, batch_size)]


def planes_to_latent(planes: torch.Tensor) -> torch.Tensor:
    """channels-last planes [3,S,S,32] -> [1,96,S,S] (the reference's tri_feat layout)."""
    S = planes.shape[1]
    return planes.permute(0, 3, 1, 2).reshape(1, 96, S, S).contiguous()


def fit_triplanes(decoder: MultiTriplane, points: torch.Tensor, occupancies: torch.Tensor, init: torch.Tensor,
                  epochs: int = 20, batch_size: int = 40000, lr: float = 1e-3, generator: Optional[torch.Generator] = None,
                  batch_fn=None):
    """The optimisation loop of train_triplane_opt (drag_utils.py:521-539) from `init` ([1,96,S,S], un-normalised) with
    the decoder's MLP frozen.  Per epoch one randperm of the points; per batch r = rand*2-1 and the offset noise, all
    from `generator` (a device torch.Generator).  `batch_fn(step) -> (idx, r, noise)` replaces them (parity runs).
    Returns (planes [3,S,S,32], losses [steps, 4] = (bce, mse, l2reg, tvreg) per step, on the device).  The host never
    waits on the device inside the loop."""
    dev = decoder.device
    points = _lib.tensor(points, torch.float32, dev, (-1, 3))
    occupancies = _lib.tensor(occupancies, torch.float32, dev, (-1,))
    n = points.shape[0]
    assert occupancies.shape[0] == n
    sched = batch_schedule(n, batch_size)
    steps = epochs * len(sched)
    opt = TriplaneAdam(prepare_planes(init.to(dev), None, None), lr=lr)
    losses = torch.zeros((steps, 4), dtype=torch.float32, device=dev)
    k = 0
    for _ in range(epochs):
        perm = None if batch_fn is not None else torch.randperm(n, generator=generator, device=dev).to(torch.int32)
        for start, cnt in sched:
            if batch_fn is not None:
                idx, r, noise = batch_fn(k)
            else:
                idx = perm[start:start + cnt]
                r = torch.rand((cnt, 3), generator=generator, device=dev) * 2 - 1
                noise = torch.randn((cnt, 3), generator=generator, device=dev)
            decoder.fit_loss_grad(opt.planes, points, occupancies, idx, r, noise, dplanes=opt.dplanes, loss_parts=losses[k, 0:2])
            opt.step(losses[k, 2:4])
            k += 1
    return opt.planes, losses


def total_loss(losses: torch.Tensor) -> torch.Tensor:
    """(bce, mse, l2reg, tvreg) rows -> the reference's summed loss per step."""
    return losses[..., 0] + PAIR_WEIGHT * losses[..., 1] + L2_WEIGHT * losses[..., 2] + TV_WEIGHT * losses[..., 3]
