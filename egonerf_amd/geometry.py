"""Geometry out of a trained density field: per-ray surface normals, accumulated weight and median depth (csrc/ego_geometry.hip,
DESIGN.md 3.5), frames of them, oriented, coloured point clouds, and triangle meshes of a density level set (csrc/ego_mesh.hip,
DESIGN.md 3.6) as binary PLY.

No reference counterpart: the reference's only geometric output is the expected depth `sum_s w_s z_s`, which lands between surfaces
wherever a ray's weight is bimodal.  Here the normal of a sample is `-grad f / |grad f|` of the density feature f (the direction of
`-grad sigma`), composited with the render's own weights, and the depth is the distance of the first sample at which the running weight
reaches a quantile - a depth that sits on a sample of the ray.
"""
from __future__ import annotations

import collections
import math
import os

import numpy as np
import torch

from . import _lib

RayGeometry = collections.namedtuple("RayGeometry", "normal acc z_median gradients")
Mesh = collections.namedtuple("Mesh", "vertices faces normals colors values")


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


# ---- triangle meshes of a density level set (csrc/ego_mesh.hip) --------------------------------------------------------
class Lattice(collections.namedtuple("Lattice", "kind n origin step radii H W c2w")):
    """A lattice of n = (n0, n1, n2) nodes, axis 0 fastest (node id = (i2 n1 + i1) n0 + i0): `box_lattice` or `panorama_lattice`."""

    @property
    def count(self) -> int:
        return self.n[0] * self.n[1] * self.n[2]

    def center(self, default) -> np.ndarray:
        """The point colours are seen from: the middle of a box, the pose's origin of a panorama (`default` without a pose)."""
        if self.kind == _lib.LATTICE_BOX:
            return (self.origin.astype(np.float64) + 0.5 * (np.asarray(self.n) - 1) * self.step.astype(np.float64)).astype(np.float32)
        return np.asarray(default, np.float32) if self.c2w is None else self.c2w[:, 3].copy()

    def struct(self, default_center=(0.0, 0.0, 0.0)) -> "_lib.LatticeStruct":
        """The ego_lattice of include/egonerf_hip.h; a panorama lattice without a pose gets the identity at `default_center`."""
        L = _lib.LatticeStruct()
        L.kind, L.n[:] = self.kind, self.n
        if self.kind == _lib.LATTICE_BOX:
            L.origin[:], L.step[:] = self.origin.tolist(), self.step.tolist()
        else:
            pose = self.c2w
            if pose is None:
                pose = np.concatenate([np.eye(3, dtype=np.float32), np.asarray(default_center, np.float32).reshape(3, 1)], 1)
            L.radii, L.H, L.W, L.c2w[:] = self.radii.data_ptr(), self.H, self.W, pose.reshape(-1).tolist()
            L.flip = 1   # (radius, row, col) is a left-handed frame: rows run down, columns clockwise seen from above
        return L


def _check_shape(n, who: str, wrap: bool) -> tuple:
    n = tuple(int(v) for v in n)
    if len(n) != 3 or any(v < 2 for v in n):
        raise ValueError(f"{who}: every axis needs at least 2 nodes, got {n}")
    if wrap and n[2] < 3:
        raise ValueError(f"{who}: the wrapping axis needs W >= 3, got {n[2]}")
    if n[0] * n[1] * n[2] >= 2 ** 31:
        raise ValueError(f"{who}: {n[0]} x {n[1]} x {n[2]} nodes: a lattice must have fewer than 2^31")
    return n


def box_lattice(lo, hi, shape) -> Lattice:
    """`shape` = (nx, ny, nz) nodes from corner `lo` to corner `hi`, both included; axes (x, y, z).  A node sits at
    fadd(origin, fmul((float) i, step)) per axis, each operation rounded once; origin = lo and step = (hi - lo) / (n - 1) are computed in
    float64 and rounded once."""
    n = _check_shape(shape, "box_lattice", False)
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"box_lattice: needs finite corners with lo < hi on every axis, got {lo.tolist()} and {hi.tolist()}")
    return Lattice(_lib.LATTICE_BOX, n, lo.astype(np.float32), ((hi - lo) / (np.asarray(n) - 1)).astype(np.float32), None, 0, 0, None)


def geometric_radii(r_near, r_far, n, device="cuda") -> torch.Tensor:
    """n radii from r_near to r_far in geometric progression (computed in float64), a float32 tensor on `device`."""
    r_near, r_far, n = float(r_near), float(r_far), int(n)
    if not (0.0 < r_near < r_far and math.isfinite(r_far)) or n < 2:
        raise ValueError(f"geometric_radii: needs 0 < r_near < r_far and n >= 2, got {r_near}, {r_far}, {n}")
    return torch.from_numpy((r_near * (r_far / r_near) ** (np.arange(n, dtype=np.float64) / (n - 1))).astype(np.float32)).to(device)


def panorama_lattice(H, W, radii, c2w=None) -> Lattice:
    """Axes (radius index, row, col), n = (len(radii), H, W): a node sits at fadd(o, fmul(radii[k], d)) with (o, d) the equirectangular
    ray of pixel (row, col) of an H x W panorama with the camera-to-world pose `c2w` [3,4] (erp_ray, normalised directions) - the pixel
    centres, so no node sits on a pole.  Without `c2w` the pose is the identity at the model's centre (at the origin for
    `mesh_from_values`).  `radii`: strictly increasing positive float32 device tensor (`geometric_radii`).  Axis 2 wraps: the cells of
    column W - 1 have column 0 as their far side, W cells along the axis.  The two polar caps, half a pixel wide, stay OPEN: a surface
    that crosses them has a boundary on rows 0 and H - 1."""
    if not torch.is_tensor(radii) or radii.dim() != 1:
        raise ValueError("panorama_lattice: radii must be a one-dimensional tensor")
    n = _check_shape((radii.numel(), H, W), "panorama_lattice", True)
    r = radii.detach().double().cpu()
    if not bool(torch.isfinite(r).all()) or not bool((r > 0).all()) or not bool((r[1:] > r[:-1]).all()):
        raise ValueError("panorama_lattice: radii must be finite, positive and strictly increasing")
    if not radii.is_cuda:
        raise RuntimeError(f"panorama_lattice: radii are on {radii.device}; the lattice is read on the HIP device (there is no CPU fallback)")
    pose = None
    if c2w is not None:
        pose = np.asarray(c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else c2w, np.float32)
        if pose.shape != (3, 4) or not np.isfinite(pose).all():
            raise ValueError(f"panorama_lattice: c2w must be a finite [3,4] pose, got shape {pose.shape}")
    return Lattice(_lib.LATTICE_PANORAMA, n, None, None, radii.detach().float().contiguous(), n[1], n[2], pose)


def _mesh_cap_bytes() -> float:
    raw = os.environ.get("EGO_MESH_MAX_MB", "")
    try:
        return float(raw or 4096) * 2 ** 20
    except ValueError:
        raise ValueError(f"EGO_MESH_MAX_MB must be a number of megabytes, not {raw!r}") from None


def _check_level(lattice, level, who: str) -> float:
    if not isinstance(lattice, Lattice):
        raise TypeError(f"{who}: lattice must come from box_lattice or panorama_lattice")
    level = float(level)
    if not math.isfinite(level):
        raise ValueError(f"{who}: level {level!r} must be finite")
    return level


def _check_workspace(lattice, who: str, with_values: bool) -> None:
    """Refuses a lattice whose workspace (ego_mesh_workspace_bytes plus, for `extract_mesh`, its values) is above EGO_MESH_MAX_MB."""
    need = int(_lib.load().ego_mesh_workspace_bytes(lattice.struct())) + (4 * lattice.count if with_values else 0)
    cap = _mesh_cap_bytes()
    if need > cap:
        raise ValueError(f"{who}: the lattice's {lattice.count} nodes need a workspace of {need / 2 ** 20:.0f} MB, above EGO_MESH_MAX_MB "
                         f"({cap / 2 ** 20:.0f}; default 4096): use a coarser lattice or raise the cap")


def _extract(L, values, level):
    """ego_mesh_count, the read-back of (V, F), ego_mesh_emit -> (vertices [V,3] float32, faces [F,3] int32) on values' device."""
    lib, st, dev = _lib.load(), _lib.stream_handle(), values.device
    nbytes = int(lib.ego_mesh_workspace_bytes(L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # (torch blocks are 512-byte aligned)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(lib.ego_mesh_count(L, values.data_ptr(), level, ws.data_ptr(), nbytes, counts.data_ptr(), st), "ego_mesh_count")
    V, F = (int(c) for c in counts.tolist())   # the one host synchronisation of an extraction: the outputs are allocated from it
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"mesh extraction: {V} vertices and {F} faces: both must stay below 2^31 (use a coarser lattice)")
    vertices, faces = torch.empty(V, 3, device=dev), torch.empty(F, 3, dtype=torch.int32, device=dev)
    if V:
        _lib.check(lib.ego_mesh_emit(L, values.data_ptr(), level, ws.data_ptr(), V, F, vertices.data_ptr(), faces.data_ptr(), st), "ego_mesh_emit")
    return vertices, faces


@_lib.device_guard
@torch.no_grad()
def _mesh_from_values(values, lattice, level):
    return _extract(lattice.struct(), values, level)


def mesh_from_values(lattice, values, level) -> Mesh:
    """The extractor alone: the surface value = level of any float32 device tensor `values` (lattice.count elements, node order) ->
    Mesh(vertices, faces, None, None, None).  A node is inside when value >= level (NaN: outside); the faces' normals point to the lower
    values.  Marching tetrahedra on the Kuhn decomposition (include/egonerf_hip.h, tests/mesh_ref.py); two calls return the same bits."""
    level = _check_level(lattice, level, "mesh_from_values")
    if not torch.is_tensor(values) or values.numel() != lattice.count:
        raise ValueError(f"mesh_from_values: values must be a tensor of {lattice.count} elements, one per node")
    _check_workspace(lattice, "mesh_from_values", False)
    if not values.is_cuda:
        raise RuntimeError(f"mesh_from_values: values are on {values.device}; the extractor runs only on the HIP device (there is no CPU fallback)")
    v, f = _mesh_from_values(values.detach().float().contiguous().view(-1), lattice, level)
    return Mesh(v, f, None, None, None)


@_lib.device_guard
@torch.no_grad()
def lattice_field(model, lattice) -> torch.Tensor:
    """sigma at every node of the lattice [count] (ego_mesh_field: the chart, the normalisation, the density feature of the full-resolution
    factored tables and feature2density in one kernel) on the model's device."""
    dev = model.density_plane_yin[0].device
    values = torch.empty(lattice.count, device=dev)
    _lib.check(_lib.load().ego_mesh_field(model.scene(), lattice.struct(model.coordinates.center.tolist()), values.data_ptr(),
                                          _lib.stream_handle()), "ego_mesh_field")
    return values


@_lib.device_guard
@torch.no_grad()
def point_gradient(model, xyz, normalize=False) -> torch.Tensor:
    """grad_xyz of the density feature at device points `xyz` [M,3] (ego_point_gradient; render_geometry's per-sample gradient, the chart
    chosen per point); normalize=True: -grad f / |grad f|, the surface normal.  0 where the gradient is 0 or not finite."""
    xyz = xyz.detach().float().contiguous()
    out = torch.empty_like(xyz)
    _lib.check(_lib.load().ego_point_gradient(model.scene(), xyz.data_ptr(), xyz.shape[0], int(bool(normalize)), out.data_ptr(),
                                              _lib.stream_handle()), "ego_point_gradient")
    return out


@torch.no_grad()
def vertex_colors(model, vertices, center, chunk=65536) -> torch.Tensor:
    """uint8 [V,3]: the stage ops at the vertices (from_cartesian, normalize_coord, compute_appfeature, renderModule), the view direction
    pointing from `center` to the vertex; `chunk` vertices at a time.  Off the hot path."""
    out = torch.empty(vertices.shape[0], 3, dtype=torch.uint8, device=vertices.device)
    c = torch.as_tensor(np.asarray(center, np.float32), device=vertices.device)
    for first in range(0, vertices.shape[0], int(chunk)):
        x = vertices[first:first + int(chunk)]
        view = torch.nn.functional.normalize(x - c, dim=-1)
        c7n = model.coordinates.normalize_coord(model.coordinates.from_cartesian(x))
        rgb = model.renderModule(x, view, model.compute_appfeature(c7n))
        out[first:first + x.shape[0]] = (rgb.clamp(0, 1) * 255).to(torch.uint8)
    return out


def extract_mesh(model, lattice, level, normals=True, colors=False, return_values=False) -> Mesh:
    """The surface sigma = level of the model's density on `lattice` -> Mesh(vertices [V,3] float32, faces [F,3] int32, normals [V,3] |
    None, colors [V,3] uint8 | None, values [count] | None), everything on the model's device.

    ego_mesh_field puts sigma on the lattice; ego_mesh_count and ego_mesh_emit extract the surface (`mesh_from_values`; between them V and
    F are read back, the one host synchronisation); normals are ego_point_gradient's -grad f / |grad f| at the vertices; colours are
    `vertex_colors` seen from the lattice's centre.  The face normals point to the lower density.  V = 0 gives empty tensors and no
    further launch.  Neither the alpha mask nor the baked node grid is read.  Two calls return the same bits."""
    level = _check_level(lattice, level, "extract_mesh")
    if normals and not model.coordinates.interval_th:
        raise NotImplementedError("extract_mesh needs the linearised exponential grid (interval_th=True): the plain exponential grid normalises r "
                                  "through a truncated logarithm, whose cell the gradient kernels do not re-derive")
    _check_workspace(lattice, "extract_mesh", True)
    dev = model.density_plane_yin[0].device
    if dev.type != "cuda":
        raise RuntimeError(f"extract_mesh: the model is on {dev}; the EgoNeRF hot path runs only on the HIP device (there is no CPU fallback)")
    if lattice.radii is not None and lattice.radii.device != dev:
        raise RuntimeError(f"extract_mesh: the lattice's radii are on {lattice.radii.device}, the model on {dev}")
    values = lattice_field(model, lattice)
    vertices, faces = _extract_on(model, lattice, values, level)
    V = vertices.shape[0]
    nrm = (point_gradient(model, vertices, True) if V else torch.empty(0, 3, device=dev)) if normals else None
    col = (vertex_colors(model, vertices, lattice.center(model.coordinates.center.tolist())) if V
           else torch.empty(0, 3, dtype=torch.uint8, device=dev)) if colors else None
    return Mesh(vertices, faces, nrm, col, values if return_values else None)


@_lib.device_guard
@torch.no_grad()
def _extract_on(model, lattice, values, level):
    return _extract(lattice.struct(model.coordinates.center.tolist()), values, level)


def export_mesh(model, path, lattice, level, **kw) -> tuple:
    """`extract_mesh(model, lattice, level, **kw)` written to `path` as a binary PLY with faces -> (V, F)."""
    m = extract_mesh(model, lattice, level, **kw)
    host = lambda t: None if t is None else t.cpu().numpy()
    write_ply(path, host(m.vertices), host(m.normals), host(m.colors), faces=host(m.faces))
    return m.vertices.shape[0], m.faces.shape[0]


def write_ply(path, xyz, normal=None, rgb=None, faces=None) -> int:
    """Binary little-endian PLY of points `xyz` [n,3] with optional `normal` [n,3] (float32 nx ny nz), `rgb` [n,3] (uint8 red green
    blue) and `faces` [F,3] (vertex indices: `element face F`, `property list uchar int vertex_indices`) -> the number of vertices
    written.  Without `faces` the file has no face element.  Plain numpy: usable without a GPU."""
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
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "".join(f"property {names[t]} {name}\n" for name, t in fields)
    face_rec = None
    if faces is not None:
        faces = np.asarray(faces)
        if faces.dtype.kind not in "iu" or faces.ndim != 2 or faces.shape[1] != 3:
            raise ValueError("write_ply: faces must be an integer array [F,3]")
        if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= n):
            raise ValueError("write_ply: a face names a vertex outside [0, n)")
        face_rec = np.empty(faces.shape[0], dtype=_PLY_FACE)
        face_rec["count"], face_rec["ids"] = 3, faces
        header += f"element face {faces.shape[0]}\nproperty list uchar int vertex_indices\n"
    with open(os.fspath(path), "wb") as fh:
        fh.write((header + "end_header\n").encode("ascii"))
        fh.write(rec.tobytes())
        if face_rec is not None:
            fh.write(face_rec.tobytes())
    return n


_PLY_FACE = np.dtype([("count", "u1"), ("ids", "<i4", (3,))])   # one triangle of `property list uchar int vertex_indices`


def read_ply(path) -> dict:
    """What `write_ply` wrote -> {"xyz": [n,3] float32, "normal": [n,3] float32 | None, "rgb": [n,3] uint8 | None}, and "faces" [F,3]
    int32 for a file with a face element (triangles only)."""
    raw = open(os.fspath(path), "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("read_ply: not a binary little-endian PLY")
    n = int(next(l for l in lines if l.startswith("element vertex ")).split()[2])
    types = {"float": "<f4", "uchar": "u1"}
    fields = [(l.split()[2], types[l.split()[1]]) for l in lines if l.startswith("property ") and not l.startswith("property list ")]
    rec = np.frombuffer(raw, dtype=np.dtype(fields), count=n, offset=end)
    pick = lambda names: np.stack([rec[k] for k in names], -1) if names[0] in rec.dtype.names else None
    out = dict(xyz=pick(("x", "y", "z")), normal=pick(("nx", "ny", "nz")), rgb=pick(("red", "green", "blue")))
    face_line = next((l for l in lines if l.startswith("element face ")), None)
    if face_line is not None:
        if "property list uchar int vertex_indices" not in lines:
            raise ValueError("read_ply: the face element must be `property list uchar int vertex_indices`")
        fr = np.frombuffer(raw, dtype=_PLY_FACE, count=int(face_line.split()[2]), offset=end + rec.nbytes)
        if fr.size and not (fr["count"] == 3).all():
            raise ValueError("read_ply: only triangles are read")
        out["faces"] = np.ascontiguousarray(fr["ids"])
    return out
