"""Geometry out of a trained density field: per-ray surface normals, accumulated weight and median depth (csrc/ego_geometry.hip,
DESIGN.md 3.5), frames of them, and oriented, coloured point clouds as binary PLY.

No reference counterpart: the reference's only geometric output is the expected depth `sum_s w_s z_s`, which lands between surfaces
wherever a ray's weight is bimodal.  Here the normal of a sample is `-grad f / |grad f|` of the density feature f (the direction of
`-grad sigma`), composited with the render's own weights, and the depth is the distance of the first sample at which the running weight
reaches a quantile - a depth that sits on a sample of the ray.
"""
from __future__ import annotations

import collections
import os

import numpy as np
import torch

from . import _lib

RayGeometry = collections.namedtuple("RayGeometry", "normal acc z_median gradients")


def _check_quantile(quantile, who: str) -> float:
    q = float(quantile)
    if not 0.0 < q < 1.0:
        raise ValueError(f"{who}: quantile {quantile!r} must lie in (0, 1)")
    return q


def _check_request(model, rays, n_coarse, n_fine, resampling, use_coarse_sample, quantile, who: str = "render_geometry"):
    """The refusals that need no library: -> (quantile, samples per ray)."""
    q = _check_quantile(quantile, who)
    if rays.dim() != 2 or rays.shape[1] < 6:
        raise IndexError(f"{who}: rays must be [N, >=6] (origin, direction), got {tuple(rays.shape)}")
    if not model.coordinates.interval_th:
        raise NotImplementedError(f"{who} needs the linearised exponential grid (interval_th=True): the plain exponential grid normalises r "
                                  "through a truncated logarithm, whose cell the gradient kernels do not re-derive")
    S = _lib.sample_count(int(n_coarse), int(n_fine), bool(resampling), bool(use_coarse_sample))
    if S < 1 or int(n_coarse) < 1:
        raise ValueError(f"{who}: no samples (n_coarse={n_coarse}, n_fine={n_fine})")
    if rays.shape[0] * S >= 2 ** 31:
        raise ValueError(f"{who}: {rays.shape[0]} rays x {S} samples: N S must be below 2^31 (render in chunks)")
    if not rays.is_cuda:
        raise RuntimeError(f"{who}: rays are on {rays.device}; the EgoNeRF hot path runs only on the HIP device (there is no CPU fallback)")
    return q, S


def render_geometry(model, rays, n_coarse, n_fine=0, resampling=False, use_coarse_sample=True, normalize=True, quantile=0.5,
                    sample_gradients=False) -> RayGeometry:
    """RayGeometry(normal [N,3], acc [N], z_median [N], gradients [N,S,3] | None) of `rays` [N,6] on the model's device.

    The samples and weights are those of the eval render with exp_sampling=True: one ego_march_density on the eval schedule, or with
    `resampling` the coarse march on the pooled tables, ego_sample_pdf_merge and the fine march - the stage sequence of
    EgoNeRF._forward_eval_ray0_distances and train._march.  The weights are taken as the march gives them, so its options hold: the alpha
    mask (use_alpha_mask), use_weight_thres, early_termination_eps, and the baked node grid where dense_density is on.  ego_ray_geometry
    then runs on the last pass's z, coords and weight; normals always come from the factored full-resolution tables.

    normal = sum_s w_s n_s with n_s = -grad f / |grad f|; normalize=True divides it by its length (0 stays 0), normalize=False leaves a
    vector of length <= acc that says how well the ray's normals agree.  acc = sum_s w_s.  z_median = z of the first sample at which the
    running weight reaches `quantile` (0.5: the median), 0 for a ray that never reaches it.  sample_gradients=True also returns grad f at
    every sample.  Runs without a graph (torch.no_grad); two calls return the same bits."""
    q, S = _check_request(model, rays, n_coarse, n_fine, resampling, use_coarse_sample, quantile)
    return _render_geometry(model, rays, int(n_coarse), int(n_fine), bool(resampling), bool(use_coarse_sample), bool(normalize), q, S,
                            bool(sample_gradients))


@_lib.device_guard
@torch.no_grad()
def march_samples(model, rays, n_coarse, n_fine=0, resampling=False, use_coarse_sample=True):
    """(z [N,S], weight [N,S], coords [N,S,4]) of the eval render's last pass for float32 device rays [N,6], N >= 1: one
    ego_march_density on the eval schedule, or the coarse march on the pooled tables, ego_sample_pdf_merge and the fine march."""
    lib, st, sc = _lib.load(), _lib.stream_handle(), model.scene()
    N, dev = rays.shape[0], rays.device
    S = _lib.sample_count(n_coarse, n_fine, resampling, use_coarse_sample)
    f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    near = float(model.near_far[0])
    sched = model._sched(n_coarse, dev).data_ptr()
    z, w, crd = f(N, S), f(N, S), f(N, S, 4)
    chk = _lib.check
    if resampling:
        zc, wc = f(N, n_coarse), f(N, n_coarse)
        chk(lib.ego_march_density(sc, rays.data_ptr(), N, n_coarse, None, sched, None, near, 1, zc.data_ptr(), None, 0, wc.data_ptr(), None, None,
                                  None, None, st), "ego_march_density")
        chk(lib.ego_sample_pdf_merge(zc.data_ptr(), wc.data_ptr(), None, N, n_coarse, n_fine, int(use_coarse_sample), z.data_ptr(), None, st),
            "ego_sample_pdf_merge")
        # fine pass: full tables and the full-resolution r grid (bit 1), as train._march
        chk(lib.ego_march_density(sc, rays.data_ptr(), N, S, z.data_ptr(), None, None, near, 2, None, None, 0, w.data_ptr(), None, crd.data_ptr(),
                                  None, None, st), "ego_march_density")
    else:
        chk(lib.ego_march_density(sc, rays.data_ptr(), N, S, None, sched, None, near, 0, z.data_ptr(), None, 0, w.data_ptr(), None, crd.data_ptr(),
                                  None, None, st), "ego_march_density")
    return z, w, crd


@_lib.device_guard
@torch.no_grad()
def ray_geometry(model, rays, z, coords, weight, normalize=True, quantile=0.5, normal=True, acc=True, z_quantile=True, gradients=False):
    """ego_ray_geometry on given samples (float32 device tensors: rays [N,6], z, weight [N,S], coords [N,S,4]) -> RayGeometry; the
    flags choose which outputs are asked for (the others are None)."""
    N, S = z.shape
    f = lambda on, *shape: torch.empty(*shape, device=z.device, dtype=torch.float32) if on else None
    out = RayGeometry(f(normal, N, 3), f(acc, N), f(z_quantile, N), f(gradients, N, S, 3))
    _lib.check(_lib.load().ego_ray_geometry(model.scene(), rays.data_ptr(), z.data_ptr(), coords.data_ptr(), weight.data_ptr(), N, S,
                                            int(bool(normalize)), float(quantile), *(_lib.ptr(t) for t in out), _lib.stream_handle()),
               "ego_ray_geometry")
    return out


def _render_geometry(model, rays, n_coarse, n_fine, resampling, use_coarse_sample, normalize, q, S, sample_gradients) -> RayGeometry:
    rays = rays[:, :6].detach().contiguous().float()
    if rays.shape[0] == 0:
        e = lambda *shape: torch.empty(*shape, device=rays.device, dtype=torch.float32)
        return RayGeometry(e(0, 3), e(0), e(0), e(0, S, 3) if sample_gradients else None)
    z, w, crd = march_samples(model, rays, n_coarse, n_fine, resampling, use_coarse_sample)
    return ray_geometry(model, rays, z, crd, w, normalize, q, gradients=sample_gradients)


def geometry_frame(model, H, W, c2w, camera="erp", focal=None, center=None, chunk=16384, **render_kw) -> dict:
    """One camera's geometry: {"normal" [H,W,3], "acc" [H,W], "z_median" [H,W], "points" [H,W,3] = o + d z_median} on the model's device.
    Rays come from `camera_rays` chunk by chunk (`chunk` rays at a time) and go through `render_geometry(**render_kw)`; a pixel's values
    do not depend on the chunking."""
    from .camera import camera_rays
    if int(chunk) < 1:
        raise ValueError("geometry_frame: chunk must be >= 1")
    if render_kw.get("sample_gradients"):
        raise ValueError("geometry_frame: sample_gradients is per sample, not per pixel; call render_geometry on the rays")
    dev = model.density_plane_yin[0].device
    n = H * W
    normal, acc, zq, pts = (torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, 3, device=dev))
    buf = torch.empty(min(int(chunk), max(n, 1)), 6, device=dev)
    for first in range(0, n, int(chunk)):
        count = min(int(chunk), n - first)
        rays = camera_rays(H, W, c2w, model=camera, focal=focal, center=center, first=first, count=count, out=buf)
        g = render_geometry(model, rays, **render_kw)
        sl = slice(first, first + count)
        normal[sl], acc[sl], zq[sl] = g.normal, g.acc, g.z_median
        pts[sl] = rays[:, :3] + rays[:, 3:6] * g.z_median[:, None]
    return dict(normal=normal.view(H, W, 3), acc=acc.view(H, W), z_median=zq.view(H, W), points=pts.view(H, W, 3))


def normal_image(normal: torch.Tensor) -> torch.Tensor:
    """uint8 [H,W,3] (or [n,3]) of device normals: 0.5 n + 0.5 through finish_frame's byte path (clamp, * 255, truncate)."""
    from .camera import finish_frame
    if not normal.is_cuda:
        raise ValueError("normal_image: normals must be a device tensor (the HIP path has no CPU fallback)")
    rgb = normal.float() * 0.5 + 0.5
    return finish_frame(rgb, torch.zeros(rgb.shape[:-1], device=rgb.device), (0.0, 1.0), palette=False)[0]


def export_point_cloud(model, c2ws, H, W, path, camera="erp", min_acc=0.5, stride=1, **render_kw) -> int:
    """Writes the oriented, coloured point cloud of the poses `c2ws` to `path` (binary PLY) and returns the number of points.

    Per pose: `geometry_frame`, then the colours of the same rays from `model.forward` (eval, exp_sampling=True, the same sampling
    arguments).  The colours are a SECOND march of every ray: export is off the hot path, and the render kernels are left as they are.
    A pixel is kept when acc >= min_acc; `stride` keeps every stride-th row and column.  min_acc below the quantile is refused: such a
    pixel may never reach the quantile and then has no z_median."""
    from .camera import camera_rays
    q = _check_quantile(render_kw.get("quantile", 0.5), "export_point_cloud")
    if not float(min_acc) >= q:
        raise ValueError(f"export_point_cloud: min_acc {min_acc} is below the quantile {q}: a pixel with acc < quantile has no z_median")
    if int(stride) < 1:
        raise ValueError("export_point_cloud: stride must be >= 1")
    chunk = int(render_kw.pop("chunk", 16384))
    fwd_kw = {k: render_kw[k] for k in ("n_coarse", "n_fine", "resampling", "use_coarse_sample") if k in render_kw}
    dev = model.density_plane_yin[0].device
    xyz, nrm, rgb = [], [], []
    for c2w in c2ws:
        fr = geometry_frame(model, H, W, c2w, camera=camera, chunk=chunk, **render_kw)
        col = torch.empty(H * W, 3, device=dev)
        for first in range(0, H * W, chunk):
            count = min(chunk, H * W - first)
            rays = camera_rays(H, W, c2w, model=camera, focal=render_kw.get("focal"), center=render_kw.get("center"), first=first, count=count,
                               device=dev)
            with torch.no_grad():
                col[first:first + count] = model(rays, is_train=False, exp_sampling=True, need_alpha=False, **fwd_kw)[0]
        keep = fr["acc"] >= float(min_acc)
        if int(stride) > 1:
            grid = torch.zeros_like(keep)
            grid[::int(stride), ::int(stride)] = True
            keep &= grid
        keep = keep.view(-1)
        xyz.append(fr["points"].view(-1, 3)[keep].cpu().numpy())
        nrm.append(fr["normal"].view(-1, 3)[keep].cpu().numpy())
        rgb.append((col[keep].clamp(0, 1) * 255).to(torch.uint8).cpu().numpy())
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros((0, 3), dt)
    return write_ply(path, cat(xyz, np.float32), cat(nrm, np.float32), cat(rgb, np.uint8))


def write_ply(path, xyz, normal=None, rgb=None) -> int:
    """Binary little-endian PLY of points `xyz` [n,3] with optional `normal` [n,3] (float32 nx ny nz) and `rgb` [n,3] (uint8 red green
    blue) -> the number of vertices written.  Plain numpy: usable without a GPU."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    cols = [xyz]
    if normal is not None:
        normal = np.asarray(normal, dtype=np.float32).reshape(-1, 3)
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        cols.append(normal)
    if rgb is not None:
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8:
            raise ValueError("write_ply: rgb must be uint8")
        rgb = rgb.reshape(-1, 3)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        cols.append(rgb)
    if any(c.shape[0] != n for c in cols):
        raise ValueError("write_ply: xyz, normal and rgb must hold the same number of points")
    rec = np.empty(n, dtype=np.dtype(fields))
    for k, (name, _) in enumerate(fields):
        rec[name] = cols[k // 3][:, k % 3]
    names = {"<f4": "float", "u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "".join(f"property {names[t]} {name}\n" for name, t in fields) + "end_header\n"
    with open(os.fspath(path), "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())
    return n


def read_ply(path) -> dict:
    """What `write_ply` wrote -> {"xyz": [n,3] float32, "normal": [n,3] float32 | None, "rgb": [n,3] uint8 | None}."""
    raw = open(os.fspath(path), "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("read_ply: not a binary little-endian PLY")
    n = int(next(l for l in lines if l.startswith("element vertex ")).split()[2])
    types = {"float": "<f4", "uchar": "u1"}
    fields = [(l.split()[2], types[l.split()[1]]) for l in lines if l.startswith("property ")]
    rec = np.frombuffer(raw, dtype=np.dtype(fields), count=n, offset=end)
    pick = lambda names: np.stack([rec[k] for k in names], -1) if names[0] in rec.dtype.names else None
    return dict(xyz=pick(("x", "y", "z")), normal=pick(("nx", "ny", "nz")), rgb=pick(("red", "green", "blue")))
