"""Mirror of triplane_decoder/visualize.py's call surface over the decode and surface kernels.

Same names, arguments and return types as the reference functions third parties call:

  create_obj(model, obj_idx, res=128, max_batch_size=50000, output_path='output.obj')      visualize.py:36-73
  create_obj_o3d(model, obj_idx, res=128, max_batch_size=50000) -> mesh                     visualize.py:76-105
  main(args=None, feature=None)                                                             visualize.py:108-128

`model` is ishapediting_amd.triplane_decoder.MultiTriplane with its `embeddings` set (drag_utils.py:295-298,
generate.py:95).  The reference decodes the res^3 grid in `max_batch_size`-point chunks with a host round trip each
(:89-95) and runs PyMCubes on the CPU; here the whole grid is one kernel launch and the level-0 surface is extracted on
the device, so `max_batch_size` is accepted and ignored.  Each function keeps its own vertex convention: create_obj
divides by 255 (:72), create_obj_o3d by res (:101).
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from . import mesh as mesh_backend
from .triplane_decoder import MultiTriplane, decode_planes_grid


def decode_grid(model: MultiTriplane, obj_idx: int, res: int) -> torch.Tensor:
    """The dense-grid half both functions share (:41-67, :79-97): logits on linspace(-1,1,res)^3 ('ij') -> [res,res,res]
    on the device."""
    model.eval()
    return decode_planes_grid(model, model._planes(obj_idx), res)


def create_obj(model: MultiTriplane, obj_idx: int, res: int = 128, max_batch_size: int = 50000,
               output_path: str = "output.obj"):
    """visualize.py:36-73: level-0 surface of the decoded grid, vertices / 255 * 2 - 1, written as Wavefront OBJ."""
    del max_batch_size
    vol = decode_grid(model, obj_idx, res)
    mesh_backend.export_obj(vol, output_path, scale_div=255.0)
    return vol


def _simplified(verts, tris, grid_res: int, cell):
    """mesh.simplify_vertex_clustering on a surface in grid coordinates of a grid_res^3 grid, cells of `cell` voxels from origin 0"""
    if cell is None or verts.shape[0] == 0 or tris.shape[0] == 0:
        return verts, tris
    dims = [int(np.floor((grid_res - 1) / float(cell))) + 1] * 3
    return mesh_backend.simplify_vertex_clustering(verts, tris, float(cell), origin=(0.0, 0.0, 0.0), dims=dims)[:2]


def create_obj_simplified(model: MultiTriplane, obj_idx: int, res: int, cell: float, output_path: str = "output.obj"):
    """create_obj with the surface reduced by quadric vertex clustering (cells of `cell` voxels) before it is written; the same
    vertex convention, / 255 * 2 - 1"""
    vol = decode_grid(model, obj_idx, res)
    verts, tris = _simplified(*mesh_backend.extract_surface(vol, 0.0), res, cell)
    mesh_backend.write_surface(output_path, verts / 255.0 * 2 - 1, tris)
    return vol


def create_obj_sparse(model: MultiTriplane, obj_idx: int, res: int, mesh_res: int, output_path: str = "output.obj", simplify=None):
    """create_obj at a mesh resolution above the decoded grid's: the dense res^3 volume only seeds the bricks of the fine grid
    (mesh.extract_surface_sparse); vertices / (mesh_res - 1) * 2 - 1, create_obj's convention (255 = 256 - 1) at that grid.
    Written by mesh.write_surface: streamed OBJ text (binary PLY if output_path ends in .ply); more than
    mesh.MAX_SPARSE_OBJ_VERTICES vertices as text raise -- no stub file.
    simplify: None, or a cell size in fine voxels: the surface is reduced by quadric vertex clustering before it is written."""
    model.eval()
    planes = model._planes(obj_idx)
    vol = decode_planes_grid(model, planes, res)
    verts, tris, info = mesh_backend.extract_surface_sparse(model, planes, mesh_res, vol)
    del info
    verts, tris = _simplified(verts, tris, mesh_res, simplify)
    mesh_backend.write_surface(output_path, verts / (mesh_res - 1) * 2 - 1, tris)
    return vol


def create_obj_o3d(model: MultiTriplane, obj_idx: int, res: int = 128, max_batch_size: int = 50000):
    """visualize.py:76-105: the mesh of the decoded grid, vertices / res * 2 - 1, NOT smoothed (get_mesh applies
    filter_smooth_simple itself, drag_utils.py:300).  Returns what mesh.BACKEND selects: an OccupancyMesh ("device"), an
    open3d.geometry.TriangleMesh built from the device surface ("open3d") or by PyMCubes ("third_party")."""
    del max_batch_size
    vol = decode_grid(model, obj_idx, res)
    return mesh_backend.volume_to_mesh(vol, res, smooth_iterations=0)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--input", type=str)
    p.add_argument("--output", type=str, required=True)
    p.add_argument("--model_path", type=str, default="models/epoch_24_decoder_loss=25.37570571899414.pt", required=False)
    p.add_argument("--res", type=int, default=128, required=False)
    return p


def main(args=None, feature=None, state_dict=None):
    """visualize.py:108-128: load the decoder (`args.model_path`), take the triplanes from `args.input` (a .npy that
    reshapes to 3x32x128x128) or from `feature`, decode at `args.res` and write `args.output`.  `state_dict` replaces the
    checkpoint file (tests, synthetic runs: no checkpoints exist offline)."""
    if args is None:
        args = build_parser().parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    model = MultiTriplane(1, input_dim=3, output_dim=1, device=device)
    model.net.load_state_dict(state_dict if state_dict is not None else torch.load(args.model_path, map_location="cpu"))
    model.eval()
    triplanes = np.load(args.input) if feature is None else feature
    triplanes = np.asarray(triplanes.detach().cpu() if torch.is_tensor(triplanes) else triplanes, dtype=np.float32)
    side = int(round((triplanes.size // 96) ** 0.5))
    triplanes = triplanes.reshape(3, 32, side, side)      # the reference hard-codes 128 (:121); any square side works here
    for i in range(3):
        model.embeddings[i] = torch.as_tensor(triplanes[[i]], device=device)
    mesh_res = getattr(args, "mesh_res", None)          # generate.py --mesh_resolution; absent or not above res: the dense path
    cell = getattr(args, "mesh_simplify", None)         # generate.py --mesh_simplify; absent: the mesh as cut
    if mesh_res is not None and int(mesh_res) > args.res:
        create_obj_sparse(model, 0, args.res, int(mesh_res), output_path=args.output, simplify=cell)
    elif cell is not None:
        create_obj_simplified(model, 0, args.res, float(cell), output_path=args.output)
    else:
        create_obj(model, 0, res=args.res, output_path=args.output)


if __name__ == "__main__":
    main()
