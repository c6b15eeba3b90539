"""Writes tests/golden/camera_rays.npz: the reference's pinhole rays, for tests/test_hip_camera_path.py.

    python tools/capture_camera_golden.py --reference /path/to/the/reference/checkout

Imports the real reference (dataLoader/ray_utils.py) with the stub modules oracle/capture_golden.py uses for its missing third-party
imports, runs its get_ray_directions, get_ray_directions_blender and get_rays on the CPU and stores inputs and outputs.  The fixture
holds data only; no reference code is copied anywhere.

kornia is not installed, so `create_meshgrid` is a stand-in with kornia's contract for `create_meshgrid(H, W,
normalized_coordinates=False)`: a float32 tensor [1, H, W, 2] whose [..., 0] is the x coordinate = the column index and whose
[..., 1] is the y coordinate = the row index (kornia.utils.create_meshgrid: "the last dimension holds x then y", `linspace(0, W - 1,
W)` by `linspace(0, H - 1, H)`).

Stored per case (`small/`: 37 x 53, fx != fy, off-centre principal point, every pixel; `big/`: 800 x 800, focal 400, default centre,
about 4096 hashed pixel indices):
  H, W, focal [2], center [2] (big: the default, stored as NaN), index [n] int64 (row-major pixel indices), poses [K, 3, 4],
  dirs/<model> [n, 3]: camera-space directions, rays/<model> [K, n, 6]: get_rays per pose, origin then direction.
Pose 0 is R = I with a translation (the world direction is then the camera-space direction exactly), the others are rotations about
all three axes with a translation.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def create_meshgrid(height, width, normalized_coordinates=True, device=None, dtype=torch.float32):
    """kornia.utils.create_meshgrid's contract for normalized_coordinates=False (see the module docstring)."""
    assert not normalized_coordinates
    xs = torch.linspace(0, width - 1, width, dtype=dtype)
    ys = torch.linspace(0, height - 1, height, dtype=dtype)
    return torch.stack(torch.meshgrid(xs, ys, indexing="ij"), dim=-1).permute(1, 0, 2).unsqueeze(0)   # [1, H, W, 2]: x, y


def rotation(ax: float, ay: float, az: float) -> np.ndarray:
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def poses() -> np.ndarray:
    p = np.zeros((3, 3, 4), np.float64)
    p[0, :, :3], p[0, :, 3] = np.eye(3), (0.125, -0.3, 0.0625)
    p[1, :, :3], p[1, :, 3] = rotation(0.3, -1.1, 2.0), (0.21, 0.07, -0.18)
    p[2, :, :3], p[2, :, 3] = rotation(-2.4, 0.6, -0.9), (-0.11, 0.19, 0.05)
    return p.astype(np.float32)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("EGONERF_REFERENCE"), help="checkout of the reference implementation")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "camera_rays.npz"))
    a = ap.parse_args()
    if not a.reference or not os.path.isdir(a.reference):
        ap.error("--reference (or EGONERF_REFERENCE) must name the reference checkout")
    sys.path.insert(0, a.reference)
    _stub("kornia", create_meshgrid=create_meshgrid)
    _stub("cv2", COLORMAP_JET=2)   # the package's __init__ imports every dataset module: the stubs of oracle/capture_golden.py
    _stub("torchvision").transforms = _stub("torchvision.transforms")
    _stub("imageio")
    _stub("plyfile", PlyData=None, PlyElement=None)
    _stub("skimage").measure = _stub("skimage.measure")
    _stub("lpips")
    from dataLoader import ray_utils as ref

    from egonerf_amd import synth
    P = poses()
    out = {}
    for case, H, W, focal, center, n_pick in (("small", 37, 53, [41.3, 39.7], [25.2, 19.6], None), ("big", 800, 800, [400.0, 400.0], None, 4096)):
        if n_pick is None:
            index = np.arange(H * W, dtype=np.int64)
        else:
            index = np.unique((synth.hash_uniform(2024, 5, n_pick) * (H * W)).astype(np.int64))
        out[f"{case}/H"], out[f"{case}/W"] = np.int64(H), np.int64(W)
        out[f"{case}/focal"] = np.asarray(focal, np.float64)
        out[f"{case}/center"] = np.asarray(center if center is not None else [np.nan, np.nan], np.float64)
        out[f"{case}/index"], out[f"{case}/poses"] = index, P
        for model, fn in (("pinhole", ref.get_ray_directions), ("pinhole_blender", ref.get_ray_directions_blender)):
            dirs = fn(H, W, focal, center)
            assert dirs.shape == (H, W, 3) and dirs.dtype == torch.float32
            out[f"{case}/dirs/{model}"] = dirs.reshape(-1, 3).numpy()[index]
            rays = []
            for p in P:
                o, d = ref.get_rays(dirs, torch.FloatTensor(p))
                rays.append(torch.cat([o, d], 1).numpy()[index])
            out[f"{case}/rays/{model}"] = np.stack(rays)
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
