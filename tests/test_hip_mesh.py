"""Mesh extraction on the GPU (csrc/ego_mesh.hip, egonerf_amd/geometry.py): the extractor against the numpy restatement of
tests/mesh_ref.py (faces as arrays, box vertices bit for bit, panorama vertices within the restatement's own float32 error), its edge cases,
the topology of what it returns, ego_mesh_field against the float64 oracle, ego_point_gradient against the oracle's autograd, and
extract_mesh / export_mesh end to end on a field whose level set is a sphere."""
import functools

import numpy as np
import pytest
import torch

from egonerf_amd import geometry, synth
from tests import geometry_ref as gref
from tests import mesh_ref as mref
from tests import ray_grad_ref as rg
from tests.helpers import make_model, make_oracle

T = torch.from_numpy
pytestmark = pytest.mark.gpu


def _device_lattice(lat):
    """The geometry.Lattice of a tests/mesh_ref.py lattice, through the public constructors; the float32 numbers are the same."""
    if lat.kind == mref.BOX:
        hi = lat.origin.astype(np.float64) + lat.step.astype(np.float64) * (np.asarray(lat.n) - 1)
        g = geometry.Lattice(geometry._lib.LATTICE_BOX, lat.n, lat.origin, lat.step, None, 0, 0, None)
        made = geometry.box_lattice(lat.origin, hi, lat.n)
        assert made.n == g.n and np.array_equal(made.origin, lat.origin)
        return g
    g = geometry.panorama_lattice(lat.H, lat.W, T(lat.radii).cuda(), lat.c2w)
    assert g.n == lat.n and np.array_equal(g.c2w, lat.c2w)
    return g


def _extract(lat, values, level):
    m = geometry.mesh_from_values(_device_lattice(lat), T(np.asarray(values, np.float32)).cuda(), level)
    assert m.normals is None and m.colors is None and m.values is None
    assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.vertices.is_cuda and m.faces.is_cuda
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- the extractor against the restatement ------------------------------------------------------------------------------------------
def test_all_256_patterns_of_one_cell():
    lat = mref.box((0.1, -0.2, 0.3), (1.1, 0.9, 1.2), (2, 2, 2))
    for pattern in range(256):
        inside = pattern >> np.arange(8) & 1                       # node id = corner bits on a 2 x 2 x 2 lattice
        values = (np.where(inside, 1.0, -1.0) * (1 + 0.1 * np.arange(8))).astype(np.float32)
        v, f = _extract(lat, values, 0.0)
        rv, rf = mref.extract(lat, values, 0.0)
        assert np.array_equal(f, rf) and _same_bits(v, rv), pattern


# 130 x 70 x 40 = 364000 nodes = 1422 workgroups of 256: more sums than the scan workgroup has threads, so a thread scans a run of them
@pytest.mark.parametrize("shape", [(3, 5, 4), (17, 9, 6), (65, 33, 3), (130, 70, 40)])
def test_random_values_on_box_lattices(shape):
    lat = mref.box((-0.7, 0.2, -1.3), (0.9, 1.45, 0.35), shape)
    values = mref.random_values(lat, 7 + shape[0])
    v, f = _extract(lat, values, 0.1)
    rv, rf = mref.extract(lat, values, 0.1)
    assert len(rf) > lat.count                                # random signs: most tetrahedra are cut
    assert np.array_equal(f, rf) and _same_bits(v, rv)


@pytest.mark.parametrize("name", sorted(mref.panorama_cases()))
def test_random_values_on_panorama_lattices(name):
    lat = mref.panorama_cases()[name]
    values = mref.random_values(lat, 1)
    v, f = _extract(lat, values, 0.0)
    r64, rf = mref.extract(lat, values, 0.0, np.float64)
    r32, _ = mref.extract(lat, values, 0.0, np.float32)
    assert np.array_equal(f, rf)
    assert (np.asarray(rf, np.int64).reshape(-1, 1) >= 0).all() and v.shape == r64.shape
    err, own = np.abs(v.astype(np.float64) - r64).max(), np.abs(r32.astype(np.float64) - r64).max()
    print(f"panorama {name}: V {len(v)} F {len(f)}  |hip - f64| {err:.3e}  |restatement f32 - f64| {own:.3e}  bound {mref.B_PANORAMA[name]:.3e}")
    assert err <= mref.B_PANORAMA[name]
    # the wrapping axis: faces exist that use vertices of both column W - 1 and column 0
    cols = mref.vertex_nodes(lat, values, 0.0)[:, 0] // (lat.n[0] * lat.n[1])
    fc = cols[f]
    assert ((fc.min(1) == 0) & (fc.max(1) == lat.W - 1)).any()


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_levels_outside_the_values_give_an_empty_mesh():
    lat = mref.box((0, 0, 0), (1, 1, 1), (5, 4, 3))
    values = mref.random_values(lat, 3)
    for level in (float(values.max()) + 1.0, float(values.min()) - 1.0, float(np.nextafter(values.max(), np.float32(np.inf)))):
        v, f = _extract(lat, values, level)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    # the largest value itself is a level that is reached: one node is inside
    v, f = _extract(lat, values, float(values.max()))
    assert len(v) > 0 and len(f) > 0


def test_values_at_the_level_nan_and_infinities():
    lat = mref.box((-1, -1, -1), (1.5, 1.25, 2), (7, 6, 5))
    values = np.round(mref.random_values(lat, 11) * 2) / 2          # multiples of 0.5: many values equal the level exactly
    rng = np.random.default_rng(5)
    special = rng.permutation(lat.count)[:60]
    values[special[:20]], values[special[20:40]], values[special[40:]] = np.nan, np.inf, -np.inf
    assert (values == 0.5).sum() > 10
    v, f = _extract(lat, values, 0.5)
    rv, rf = mref.extract(lat, values, 0.5)
    assert len(rf) > 0 and np.array_equal(f, rf) and _same_bits(v, rv)
    assert np.isfinite(v).all()
    again_v, again_f = _extract(lat, values, 0.5)
    assert _same_bits(v, again_v) and np.array_equal(f, again_f)    # two calls, the same bits


# ---- topology of the device result ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lo,hi,field,chi", [
    ((9, 7, 11), (-1, -1.1, -0.9), (1.05, 1, 1.1), mref.sphere((0.03, -0.02, 0.05), 0.7), 2),
    ((13, 11, 7), (-1.3, -1.2, -0.6), (1.25, 1.3, 0.55), mref.torus((0.02, -0.03, 0.01), 0.75, 0.33), 0),
])
def test_closed_surfaces(shape, lo, hi, field, chi):
    lat = mref.box(lo, hi, shape)
    value, outward = field
    v, f = _extract(lat, value(mref.positions(lat, np.float64)).astype(np.float32), 0.0)
    t = mref.topology(f, len(v))
    assert t["consistent"] and len(t["boundary"]) == 0 and t["all_used"] and t["chi"] == chi, t
    ok, judged = mref.winding_agrees(v, f, outward)
    assert ok and judged > 0.9 * len(f)


def test_closed_surface_on_a_lattice_whose_scan_runs_are_long():
    """200 x 120 x 100 nodes = 9375 workgroup sums: a thread of the scan owns a run of 10, more than the 8 it walks at a time.  The
    restatement would take too long here; a wrong offset anywhere shows as a vertex used twice or never, or as an open edge."""
    lat = mref.box((-1, -1.1, -0.9), (1.05, 1, 1.1), (200, 120, 100))
    c, R = np.array([0.03, -0.02, 0.05]), 0.7
    value, outward = mref.sphere(c, R)
    values = value(mref.positions(lat, np.float64)).astype(np.float32)
    v, f = _extract(lat, values, 0.0)
    t = mref.topology(f, len(v))
    assert t["consistent"] and len(t["boundary"]) == 0 and t["all_used"] and t["chi"] == 2, {k: x for k, x in t.items() if k != "boundary"}
    assert len(v) == int(mref.POPCOUNT8[mref.classify(lat, values, 0.0)[1]].sum())
    assert np.abs(np.linalg.norm(v - c, axis=1) - R).max() <= np.linalg.norm(lat.step)
    assert mref.winding_agrees(v, f, outward)[0]


def test_panorama_surface_wraps_and_leaves_the_caps_open():
    lat = mref.panorama(7, 9, mref.geometric_radii(0.3, 3.0, 8), mref.skew_pose())
    c = lat.c2w[:, 3].astype(np.float64) + np.array([0.2, -0.3, 0.25])
    value, outward = mref.sphere(c, 1.1)
    values = value(mref.positions(lat, np.float64)).astype(np.float32)
    v, f = _extract(lat, values, 0.0)
    t = mref.topology(f, len(v))
    assert t["consistent"] and t["all_used"] and t["chi"] == 0, t
    rows = mref.vertex_nodes(lat, values, 0.0) // lat.n[0] % lat.n[1]
    b = t["boundary"]
    assert len(b) >= 2 * lat.W and ((rows[b] == 0).all((1, 2)) | (rows[b] == lat.H - 1).all((1, 2))).all()
    assert mref.winding_agrees(v, f, outward)[0]


# ---- the field on a lattice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mref.FIELD_CASES)
def test_field_against_the_oracle(case):
    cfg, w, *_ = rg.case_inputs(case)
    o64 = make_oracle(cfg, w, dtype=torch.float64)
    model = make_model(cfg, w, "cuda")
    for name, lat in mref.field_lattices(o64).items():
        s64, yang, keep = mref.oracle_sigma(o64, lat)
        assert 0 < int(yang.sum()) < yang.numel(), "both charts must occur"
        assert int((~keep).sum()) <= mref.MOST_LEFT_OUT * lat.count
        hip = geometry.lattice_field(model, _device_lattice(lat)).cpu().double()
        assert hip.shape == (lat.count,) and bool(torch.isfinite(hip).all())
        scale = float(s64.abs().max())
        err = float((hip - s64)[keep].abs().max()) / scale
        print(f"field {case} {name}: nodes {lat.count}  left out {int((~keep).sum())}  max sigma {scale:.3e}  |hip - f64| / max {err:.3e}  "
              f"bound {mref.B_FIELD:.2e}")
        assert scale > 0 and err <= mref.B_FIELD


# ---- gradients at points ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gradient_case(grid):
    cfg = (synth.SceneConfig(n_voxel=20 ** 3) if grid is None
           else synth.SceneConfig(n_voxel=20 ** 3, grid=list(grid), density_n_comp=(4, 4, 4), app_n_comp=(4, 4, 4)))
    w = synth.make_weights(cfg, seed=1234)
    o64 = make_oracle(cfg, w, dtype=torch.float64)
    xyz, _ = rg.hand_placed_points(o64, per_chart=129)
    xyz = xyz[np.random.default_rng(2).permutation(len(xyz))]      # yin-table and yang-table points mixed
    x = T(xyz)
    yang = o64.from_cartesian(x.double())[:, 6] != 0               # the chart the kernel must choose
    assert float(o64.yin_margin(x.double()).abs().min()) > 1e-4    # ... with no point near a chart boundary
    g64, _ = rg.sample_grad_reference(o64, x, yang, torch.ones(len(x)), torch.zeros(len(x), cfg.app_dim))
    return make_model(cfg, w, "cuda"), x.cuda(), yang, g64


@pytest.mark.parametrize("grid", [None, (6, 5, 8), (1100, 5, 6)])   # 1101 LUT entries: beyond the kernel's LDS copy
@pytest.mark.parametrize("M", [1, 3, 64, 257])
def test_point_gradient(grid, M):
    model, x, yang, g64 = _gradient_case(grid)
    x, g64 = x[:M].contiguous(), g64[:M]
    scale = float(_gradient_case(grid)[3].abs().max())
    raw = geometry.point_gradient(model, x)
    unit = geometry.point_gradient(model, x, normalize=True)
    assert raw.shape == unit.shape == (M, 3)
    err = float((raw.cpu().double() - g64).abs().max())
    length = g64.norm(dim=-1, keepdim=True)     # 0 at a point where every plane's relu is dead: n = 0 there
    want = torch.where(length > 0, -g64 / length.clamp(min=1e-300), torch.zeros_like(g64))
    err_n = float((unit.cpu().double() - want).abs().max())
    print(f"grid {grid} M {M}: |hip - f64| {err / scale:.3e} relative to max |g64| {scale:.3e}, normalised {err_n:.3e} (bound {gref.B_KERNEL:.1e})")
    assert scale > 0 and err <= gref.B_KERNEL * scale and err_n <= gref.B_KERNEL
    if M >= 64:
        assert 0 < int(yang[:M].sum()) < M, "both charts must occur"
        assert bool((unit[(length[:, 0] == 0).cuda()].contiguous().view(torch.int32) == 0).all())   # +0.0 where the gradient is 0
    assert torch.equal(raw, geometry.point_gradient(model, x)) and torch.equal(unit, geometry.point_gradient(model, x, normalize=True))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _radial_weights(cfg, seed=1234):
    """Only the plane whose line runs along r is non-zero: a constant plane channel times a line profile that falls with r, the same on
    both charts.  The density is then a falling function of r alone, and a level set is a sphere around the centre."""
    w = dict(synth.make_weights(cfg, seed=seed))
    for g in ("yin", "yang"):
        for i in range(3):
            p, l = w[f"density_plane_{g}.{i}"], w[f"density_line_{g}.{i}"]
            C, n_r = l.shape[1], cfg.grid[0]
            if i < 2:
                w[f"density_plane_{g}.{i}"] = np.zeros_like(p)
            else:
                profile = (1 + np.arange(C)[:, None] / C) / C * (n_r - np.arange(n_r)[None, :]) / n_r     # [C, n_r], falling with r
                w[f"density_plane_{g}.{i}"] = np.ones_like(p)
                w[f"density_line_{g}.{i}"] = profile.astype(np.float32)[None, :, :, None].copy()
    return w


@functools.lru_cache(maxsize=None)
def _sphere_scene():
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = _radial_weights(cfg)
    o64 = make_oracle(cfg, w, dtype=torch.float64)
    c, R = o64.center.double().numpy(), 1.9
    with torch.no_grad():
        probe = T(c + np.array([[R, 0.0, 0.0]]))
        level = float(o64.feature2density(o64.density_feature(o64.normalize_coord(o64.from_cartesian(probe), downsample=None))))
    lo, hi, shape = c + np.array([-2.6, -2.4, -2.7]), c + np.array([2.5, 2.7, 2.45]), (15, 13, 17)
    lattice = geometry.box_lattice(lo, hi, shape)
    model = make_model(cfg, w, "cuda")
    return model, lattice, level, c, R, float(np.linalg.norm((hi - lo) / (np.asarray(shape) - 1)))


def test_extract_mesh_of_a_sphere():
    model, lattice, level, c, R, diagonal = _sphere_scene()
    m = model.extract_mesh(lattice, level, return_values=True)
    assert m.colors is None and m.values.shape == (lattice.count,) and m.normals.shape == m.vertices.shape
    v, f, n = m.vertices.cpu().numpy().astype(np.float64), m.faces.cpu().numpy(), m.normals.cpu().numpy().astype(np.float64)
    t = mref.topology(f, len(v))
    assert t["consistent"] and len(t["boundary"]) == 0 and t["all_used"] and t["chi"] == 2, t
    r = np.linalg.norm(v - c, axis=1)
    print(f"sphere: V {len(v)} F {len(f)}  | |v - c| - R | <= {np.abs(r - R).max():.3e} (cell diagonal {diagonal:.3e})")
    assert np.abs(r - R).max() <= diagonal                          # a vertex lies on an edge whose ends bracket R
    radial = (v - c) / r[:, None]
    err = np.abs(n - radial).max()                                  # the density falls with r: -grad f points outwards
    print(f"sphere: |normal - r^| {err:.3e} (bound {gref.B_KERNEL:.1e})")
    assert err <= gref.B_KERNEL
    fn, _ = mref.face_normals(v, f)
    live = np.linalg.norm(fn, axis=1) > 1e-12
    assert live.sum() > 0.9 * len(f) and ((fn[live][:, None, :] * n[f[live]]).sum(-1) > 0).all()   # the winding agrees with the normals
    # the values are the field, the mesh is the extractor on them
    alone = geometry.mesh_from_values(lattice, m.values, level)
    assert torch.equal(alone.vertices, m.vertices) and torch.equal(alone.faces, m.faces)
    assert torch.equal(m.values, geometry.lattice_field(model, lattice))
    again = geometry.extract_mesh(model, lattice, level)
    assert again.values is None and torch.equal(again.vertices, m.vertices) and torch.equal(again.normals, m.normals)
    # no surface: empty tensors
    empty = geometry.extract_mesh(model, lattice, float(m.values.max()) + 1.0, colors=True)
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.normals.shape == (0, 3) and empty.colors.shape == (0, 3)
    assert empty.colors.dtype == torch.uint8 and empty.faces.dtype == torch.int32


def test_colors_and_export(tmp_path):
    model, lattice, level, c, R, _ = _sphere_scene()
    m = geometry.extract_mesh(model, lattice, level, normals=False, colors=True)
    assert m.normals is None and m.colors.dtype == torch.uint8 and m.colors.shape == m.vertices.shape
    with torch.no_grad():   # the stage ops by hand, all vertices at once (extract_mesh works in chunks)
        view = torch.nn.functional.normalize(m.vertices - T(lattice.center(c).astype(np.float32)).cuda(), dim=-1)
        c7n = model.coordinates.normalize_coord(model.coordinates.from_cartesian(m.vertices))
        rgb = model.renderModule(m.vertices, view, model.compute_appfeature(c7n))
    want = (rgb.clamp(0, 1) * 255).to(torch.uint8)
    assert int((m.colors.int() - want.int()).abs().max()) <= 1 and int(want.max()) > int(want.min())
    small = geometry.vertex_colors(model, m.vertices, lattice.center(c), chunk=37)
    assert int((small.int() - want.int()).abs().max()) <= 1
    path = tmp_path / "sphere.ply"
    V, F = geometry.export_mesh(model, path, lattice, level, colors=True)
    back = geometry.read_ply(path)
    full = geometry.extract_mesh(model, lattice, level, colors=True)
    assert (V, F) == (m.vertices.shape[0], m.faces.shape[0]) == (len(back["xyz"]), len(back["faces"]))
    assert np.array_equal(back["faces"], m.faces.cpu().numpy()) and np.array_equal(back["xyz"], m.vertices.cpu().numpy())
    assert np.array_equal(back["normal"], full.normals.cpu().numpy()) and np.array_equal(back["rgb"], full.colors.cpu().numpy())
