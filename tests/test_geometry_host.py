"""Host side of the ray geometry (no GPU): write_ply round trips, the refusals of egonerf_amd/geometry.py before the library is loaded,
tests/geometry_ref.py's restatement on a field whose normals are known in closed form, the quantile depth on hand-made weights, and
the new symbol of the C ABI."""
import re
import types

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, geometry, synth
from tests import geometry_ref as gref
from tests import ray_grad_ref as rg
from tests.helpers import make_oracle

T = torch.from_numpy


# ---- write_ply ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_normal,with_rgb", [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("n", [0, 1, 37])
def test_write_ply_round_trip(tmp_path, with_normal, with_rgb, n):
    rng = np.random.default_rng(n)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    normal = rng.normal(size=(n, 3)).astype(np.float32) if with_normal else None
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.uint8) if with_rgb else None
    path = tmp_path / "p.ply"
    assert geometry.write_ply(path, xyz, normal, rgb) == n
    raw = path.read_bytes()
    props = ["float x", "float y", "float z"] + ["float nx", "float ny", "float nz"] * with_normal + ["uchar red", "uchar green", "uchar blue"] * with_rgb
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "".join(f"property {p}\n" for p in props) + "end_header\n"
    assert raw.startswith(header.encode("ascii"))
    stride = 12 + 12 * with_normal + 3 * with_rgb
    assert len(raw) == len(header) + n * stride
    if n:   # the first vertex, byte for byte
        first = xyz[0].astype("<f4").tobytes() + (normal[0].astype("<f4").tobytes() if with_normal else b"") + (rgb[0].tobytes() if with_rgb else b"")
        assert raw[len(header):len(header) + stride] == first
    back = geometry.read_ply(path)
    assert np.array_equal(back["xyz"], xyz) and back["xyz"].shape == (n, 3)
    for key, want in (("normal", normal), ("rgb", rgb)):
        assert (back[key] is None) if want is None else np.array_equal(back[key], want)


def test_write_ply_refuses_mismatched_input(tmp_path):
    with pytest.raises(ValueError, match="same number of points"):
        geometry.write_ply(tmp_path / "p.ply", np.zeros((3, 3)), normal=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="uint8"):
        geometry.write_ply(tmp_path / "p.ply", np.zeros((3, 3)), rgb=np.zeros((3, 3)))


# ---- refusals, before the library is loaded -------------------------------------------------------------------------------------------
def _stub(interval_th=True):
    return types.SimpleNamespace(coordinates=types.SimpleNamespace(interval_th=interval_th))


def test_refusals_before_the_library_is_loaded(monkeypatch, tmp_path):
    def no_load():
        raise AssertionError("the library must not be loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    rays = T(synth.make_rays(4, seed=1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.render_geometry(_stub(), rays, n_coarse=8)
    with pytest.raises(NotImplementedError, match="plain exponential grid"):
        geometry.render_geometry(_stub(interval_th=False), rays, n_coarse=8)
    many = torch.empty(2 ** 22, 6, device="meta")
    with pytest.raises(ValueError, match="below 2\\^31"):
        geometry.render_geometry(_stub(), many, n_coarse=512)
    with pytest.raises(ValueError, match="below 2\\^31"):
        geometry.render_geometry(_stub(), many, n_coarse=256, n_fine=256, resampling=True)
    for q in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="quantile"):
            geometry.render_geometry(_stub(), rays, n_coarse=8, quantile=q)
    with pytest.raises(ValueError, match="below the quantile"):
        geometry.export_point_cloud(None, [], 8, 16, tmp_path / "x.ply", min_acc=0.4)
    with pytest.raises(ValueError, match="below the quantile"):
        geometry.export_point_cloud(None, [], 8, 16, tmp_path / "x.ply", min_acc=0.5, quantile=0.7)
    with pytest.raises(ValueError, match="device tensor"):
        geometry.normal_image(torch.zeros(2, 2, 3))
    assert not (tmp_path / "x.ply").exists()


# ---- the restatement on a field with known normals ------------------------------------------------------------------------------------
def _radial_field(cfg, seed=1234):
    """Density tables constant along theta^ and phi^ and increasing in r^, positive everywhere: f = f(r^) increasing, so grad f points
    radially outwards and n = -grad f / |grad f| is the inward radial unit vector, on both charts."""
    w = dict(synth.make_weights(cfg, seed=seed))
    n_r = cfg.grid[0]
    ramp = lambda C: (0.5 + np.arange(n_r)[None, :] / n_r * (1 + np.arange(C)[:, None] / C)).astype(np.float32)   # [C, n_r], increasing in r
    for g in ("yin", "yang"):
        for i in range(3):
            p, l = w[f"density_plane_{g}.{i}"], w[f"density_line_{g}.{i}"]
            C = p.shape[1]
            if i < 2:    # planes 0, 1 span (r, theta) / (r, phi) with r along W; their lines span phi / theta
                w[f"density_plane_{g}.{i}"] = np.broadcast_to(ramp(C)[None, :, None, :], p.shape).copy()
                w[f"density_line_{g}.{i}"] = np.ones_like(l)
            else:        # plane 2 spans (theta, phi); its line spans r
                w[f"density_plane_{g}.{i}"] = np.ones_like(p)
                w[f"density_line_{g}.{i}"] = ramp(C)[None, :, :, None].copy()
    return w


@pytest.mark.parametrize("grid", [None, [6, 5, 8]])
def test_restatement_on_a_radial_field(grid):
    cfg = synth.SceneConfig(n_voxel=20 ** 3) if grid is None else synth.SceneConfig(n_voxel=20 ** 3, grid=grid, density_n_comp=(4, 4, 4))
    o = make_oracle(cfg, _radial_field(cfg), dtype=torch.float64)
    xyz, yang = rg.hand_placed_points(o)
    M = len(yang)
    assert 0 < int(yang.sum()) < M
    rays = torch.cat([T(xyz).double(), T(synth.make_rays(M, seed=9))[:, 3:].double()], 1)
    z, w = torch.zeros(M, 1, dtype=torch.float64), torch.full((M, 1), 0.75, dtype=torch.float64)
    inward = -(T(xyz).double() - o.center.double())
    inward = inward / inward.norm(dim=-1, keepdim=True)
    for normalize in (True, False):
        normal, acc, zq, g, cum = gref.geometry_reference(o, rays, z, w, T(yang), normalize, 0.5)
        assert float(g.norm(dim=-1).min()) > 0
        assert float((normal - inward * (1.0 if normalize else 0.75)).abs().max()) <= 1e-12
        assert torch.equal(acc, w[:, 0]) and torch.equal(cum, w) and torch.equal(zq, z[:, 0])
    # several samples along a ray through the centre: the same inward normal at every sample, |normal| = acc without normalisation
    d = inward[:4]
    ray = torch.cat([o.center.double()[None] - d * 8.0, d], 1)          # starts 8 units out, looks at the centre
    zs = torch.tensor([[1.0, 2.5, 4.0, 5.5]], dtype=torch.float64).repeat(4, 1)
    ws = torch.tensor([[0.1, 0.2, 0.0, 0.3]], dtype=torch.float64).repeat(4, 1)
    with torch.no_grad():
        chart = o.from_cartesian((ray[:, None, :3] + ray[:, None, 3:] * zs[..., None]))[..., 6] != 0
    normal, acc, zq, g, cum = gref.geometry_reference(o, ray, zs, ws, chart, False, 0.5)
    assert float((normal - d * 0.6).abs().max()) <= 1e-12 and float((acc - 0.6).abs().max()) <= 1e-15
    assert torch.equal(zq, torch.full((4,), 5.5, dtype=torch.float64))


def test_quantile_depth_on_hand_made_weights():
    z = torch.tensor([[1.0, 2.0, 3.0, 4.0]] * 5, dtype=torch.float64)
    w = torch.tensor([[0.25, 0.25, 0.25, 0.125],     # reaches 0.5 exactly at sample 1
                      [0.125, 0.125, 0.125, 0.0625],  # never reaches it
                      [0.5, 0.0, 0.0, 0.0],           # reaches it exactly at sample 0
                      [0.75, 0.125, 0.0, 0.0],        # passes it at sample 0
                      [0.0, 0.0, 0.0, 0.625]], dtype=torch.float64)   # only at the last sample
    want = torch.tensor([2.0, 0.0, 1.0, 1.0, 4.0], dtype=torch.float64)
    assert torch.equal(gref.quantile_depth(z, w.cumsum(-1), 0.5), want)
    assert torch.equal(gref.quantile_depth(z, w.cumsum(-1), 0.875), torch.tensor([4.0, 0.0, 0.0, 2.0, 0.0], dtype=torch.float64))
    # through geometry_reference (any field): z_quantile and cum are those of the weights
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    o = make_oracle(cfg, synth.make_weights(cfg, seed=1234), dtype=torch.float64)
    rays = T(synth.make_rays(5, seed=3)).double()
    _, acc, zq, _, cum = gref.geometry_reference(o, rays, z, w, torch.zeros(5, 4, dtype=torch.bool), True, 0.5)
    assert torch.equal(zq, want) and torch.equal(cum, w.cumsum(-1)) and torch.equal(acc, w.sum(-1))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_declared_and_bound():
    assert "ego_ray_geometry" in _lib.header_symbols() and "ego_ray_geometry" in _lib.PROTOTYPES
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib.os.path.dirname(_lib.os.path.abspath(_lib.__file__))), "include", "egonerf_hip.h")).read()
    assert "#define EGO_ABI_VERSION 17" in hdr
    decl = re.search(r"\bint ego_ray_geometry\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert decl, "ego_ray_geometry is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    restype, argtypes = _lib.PROTOTYPES["ego_ray_geometry"]
    assert len(params) == len(argtypes) == 14 and restype is _lib.C.c_int
    # pointers, integers and the float line up with the declaration
    kinds = {"*": _lib.P, "int64_t": _lib.I64, "int32_t": _lib.I32, "float": _lib.F32}
    for p, a in zip(params, argtypes):
        want = _lib.SP if "ego_scene" in p else next(v for k, v in kinds.items() if k in p)
        assert a is want, (p, a)
    from egonerf_amd import build
    assert "ego_geometry.hip" in build.SOURCES and build.EXTRA_FLAGS["ego_geometry.hip"] == ["-fno-slp-vectorize"]
    assert "ego_vm_grad.h" in build.HEADERS
    from egonerf_amd.model import EgoNeRF
    assert callable(EgoNeRF.render_geometry)
