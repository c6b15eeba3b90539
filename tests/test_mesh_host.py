"""Host side of the mesh extraction (no GPU): the restatement tests/mesh_ref.py on analytic spheres and tori (closed,
consistently wound, the right Euler characteristic, normals to the outside), on a panorama lattice with its wrapping seam, on all 256
corner patterns of one cell; PLY files with faces; the refusals of egonerf_amd/geometry.py; the new symbols of the C ABI."""
import types

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, geometry
from tests import mesh_ref as mref


def _surface(lat, field):
    value, outward = field
    values = value(mref.positions(lat, np.float64)).astype(np.float32)
    v, f = mref.extract(lat, values, 0.0)
    return values, v, f, outward


# ---- the restatement on analytic fields -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lo,hi,field,chi", [
    ((9, 7, 11), (-1, -1.1, -0.9), (1.05, 1, 1.1), mref.sphere((0.03, -0.02, 0.05), 0.7), 2),
    ((11, 9, 7), (-1, -1.1, -0.9), (1.05, 1, 1.1), mref.sphere((-0.1, 0.07, 0.02), 0.55), 2),
    ((13, 11, 7), (-1.3, -1.2, -0.6), (1.25, 1.3, 0.55), mref.torus((0.02, -0.03, 0.01), 0.75, 0.33), 0),
])
def test_closed_surfaces_in_a_box(shape, lo, hi, field, chi):
    lat = mref.box(lo, hi, shape)
    values, v, f, outward = _surface(lat, field)
    inside = values >= 0
    # strictly inside the lattice: no inside node on its hull
    i = np.stack(mref.node_index(lat), -1)
    assert not inside[((i == 0) | (i == np.asarray(lat.n) - 1)).any(1)].any() and inside.any()
    t = mref.topology(f, len(v))
    assert t["consistent"] and len(t["boundary"]) == 0 and t["all_used"], t   # every edge in exactly two faces, once in each direction
    assert t["chi"] == chi, t
    ok, judged = mref.winding_agrees(v, f, outward)
    assert ok and judged > 0.9 * len(f)


def test_panorama_lattice_wraps_and_leaves_the_caps_open():
    lat = mref.panorama(7, 9, mref.geometric_radii(0.3, 3.0, 8), mref.skew_pose())
    centre = lat.c2w[:, 3].astype(np.float64)
    c, R = centre + np.array([0.2, -0.3, 0.25]), 1.1
    assert np.linalg.norm(c - centre) < R                                    # the sphere contains the lattice's centre
    assert lat.radii[0] < R - np.linalg.norm(c - centre) and R + np.linalg.norm(c - centre) < lat.radii[-1]
    values, v, f, outward = _surface(lat, mref.sphere(c, R))
    t = mref.topology(f, len(v))
    assert t["consistent"] and t["all_used"] and t["chi"] == 0, t              # a sphere less two caps: an annulus
    ends = mref.vertex_nodes(lat, values, 0.0)
    rows = ends // lat.n[0] % lat.n[1]
    cols = ends // (lat.n[0] * lat.n[1])
    b = t["boundary"]
    assert len(b) >= 2 * lat.W                                                 # a ring around each open cap, at least one edge per cell
    assert set(rows[b].reshape(-1).tolist()) <= {0, lat.H - 1}
    assert ((rows[b] == 0).all((1, 2)) | (rows[b] == lat.H - 1).all((1, 2))).all()
    # the seam is closed: vertices on edges between column W - 1 and column 0 exist and none of them is on a boundary edge away from a cap
    seam = (cols.min(1) == 0) & (cols.max(1) == lat.W - 1)
    assert seam.any()
    assert mref.winding_agrees(v, f, outward)[0]
    # the same lattice without the wrap would leave the seam open: the flag is what closes it
    assert not np.array_equal(mref.neighbour(lat, 4)[1], mref.neighbour(lat._replace(kind=mref.BOX, origin=np.zeros(3, np.float32),
                                                                                  step=np.ones(3, np.float32)), 4)[1])


def _linear_gradient(p, f):
    """The gradient of the linear function through values f [4] at points p [4,3]."""
    return np.linalg.solve(p[1:] - p[0], f[1:] - f[0])


@pytest.mark.parametrize("kind", ["box", "panorama"])
def test_all_256_patterns_of_one_cell(kind):
    lat = (mref.box((0.1, -0.2, 0.3), (1.1, 0.9, 1.2), (2, 2, 2)) if kind == "box"
           else mref.panorama(2, 3, mref.geometric_radii(1.0, 1.5, 2), mref.skew_pose()))
    pos = mref.positions(lat, np.float64)
    cell = 0   # the cell over node 0; the panorama lattice has two more around the wrapping axis, which the count includes
    corner = [int(mref.neighbour(lat, b)[0][cell]) for b in range(8)]
    for pattern in range(256):
        values = np.full(lat.count, -1.0, np.float32)
        for b in range(8):
            if pattern >> b & 1:
                values[corner[b]] = 1.0
        v, f = mref.extract(lat, values, 0.0, np.float64)
        inside = values >= 0
        cells = np.nonzero(mref.neighbour(lat, 7)[1])[0]
        want, k = 0, 0
        for c in cells:
            ids = [int(mref.neighbour(lat, b)[0][c]) for b in range(8)]
            for t in range(6):
                tc = [ids[b] for b in mref.tet_corners(t)]
                n_in = int(inside[tc].sum())
                n_tri = {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n_in]
                want += n_tri
                g = _linear_gradient(pos[tc], values[tc].astype(np.float64)) if n_tri else None
                for tri in f[k:k + n_tri]:   # faces come in (cell, tetrahedron, triangle) order
                    n = np.cross(v[tri[1]] - v[tri[0]], v[tri[2]] - v[tri[0]])
                    assert np.linalg.norm(n) > 1e-9 and n @ -g > 0, (pattern, c, t)
                k += n_tri
        assert len(f) == want == k
        if len(f):
            t = mref.topology(f, len(v))
            assert t["consistent"] and t["all_used"]
        else:
            assert len(v) == 0


def test_vertex_rules():
    lat = mref.box((0, 0, 0), (1, 1, 1), (2, 2, 2))
    values = np.array([1, 0, 3, np.nan, -1, np.inf, 0.5, -np.inf], np.float32)   # level 1: node 0 is inside (value == level), NaN outside
    inside, flags, off = mref.classify(lat, values, 1.0)
    assert inside.tolist() == [True, False, True, False, False, True, False, False]
    v, f = mref.extract(lat, values, 1.0)
    ends = mref.vertex_nodes(lat, values, 1.0)
    assert (np.diff(ends[:, 0]) >= 0).all()                                        # vertex ids increase with the owner's node id
    pos = mref.positions(lat)
    for (a, b), p in zip(ends, v):
        fa, fb = values[a], values[b]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = (np.float32(1) - fa) / (fb - fa)
        t = np.clip(t, 0, 1) if np.isfinite(t) else np.float32(0.5)
        assert np.array_equal(p, pos[a] + t * (pos[b] - pos[a]))
        if not np.isfinite(fa) or not np.isfinite(fb):
            assert t in (0.0, 0.5, 1.0)
    assert v.dtype == np.float32 and f.dtype == np.int32


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_normal,with_rgb", [(False, False), (True, True)])
@pytest.mark.parametrize("n,F", [(0, 0), (5, 0), (37, 61)])
def test_ply_with_faces_round_trip(tmp_path, with_normal, with_rgb, n, F):
    rng = np.random.default_rng(n + F)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    normal = rng.normal(size=(n, 3)).astype(np.float32) if with_normal else None
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.uint8) if with_rgb else None
    faces = rng.integers(0, max(n, 1), size=(F, 3)).astype(np.int32)
    path = tmp_path / "m.ply"
    assert geometry.write_ply(path, xyz, normal, rgb, faces=faces) == n
    raw = path.read_bytes()
    props = ["float x", "float y", "float z"] + ["float nx", "float ny", "float nz"] * with_normal + ["uchar red", "uchar green", "uchar blue"] * with_rgb
    header = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "".join(f"property {p}\n" for p in props) +
              f"element face {F}\nproperty list uchar int vertex_indices\nend_header\n")
    stride = 12 + 12 * with_normal + 3 * with_rgb
    assert raw.startswith(header.encode("ascii")) and len(raw) == len(header) + n * stride + F * 13
    if F:
        assert raw[len(header) + n * stride:][:13] == b"\x03" + faces[0].astype("<i4").tobytes()
    back = geometry.read_ply(path)
    assert np.array_equal(back["xyz"], xyz) and np.array_equal(back["faces"], faces) and back["faces"].shape == (F, 3)
    assert back["faces"].dtype == np.int32
    for key, want in (("normal", normal), ("rgb", rgb)):
        assert (back[key] is None) if want is None else np.array_equal(back[key], want)


def test_ply_without_faces_is_unchanged(tmp_path):
    rng = np.random.default_rng(3)
    xyz, normal = rng.normal(size=(9, 3)).astype(np.float32), rng.normal(size=(9, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(9, 3)).astype(np.uint8)
    geometry.write_ply(tmp_path / "a.ply", xyz, normal, rgb)
    geometry.write_ply(tmp_path / "b.ply", xyz, normal, rgb, faces=None)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 9\n" + "".join(f"property float {k}\n" for k in ("x", "y", "z", "nx", "ny", "nz")) +
              "".join(f"property uchar {k}\n" for k in ("red", "green", "blue")) + "end_header\n")
    body = b"".join(xyz[i].tobytes() + normal[i].tobytes() + rgb[i].tobytes() for i in range(9))
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes() == header.encode("ascii") + body
    assert set(geometry.read_ply(tmp_path / "a.ply")) == {"xyz", "normal", "rgb"}    # no "faces" key without a face element


def test_ply_refuses_bad_faces(tmp_path):
    xyz = np.zeros((4, 3), np.float32)
    for bad, what in ((np.zeros((2, 4), np.int32), "integer array"), (np.zeros((2, 3), np.float32), "integer array"),
                      (np.array([[0, 1, 4]], np.int32), "outside"), (np.array([[0, -1, 2]], np.int32), "outside")):
        with pytest.raises(ValueError, match=what):
            geometry.write_ply(tmp_path / "x.ply", xyz, faces=bad)
    assert not (tmp_path / "x.ply").exists()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _stub(interval_th=True):
    return types.SimpleNamespace(coordinates=types.SimpleNamespace(interval_th=interval_th, center=torch.zeros(3)),
                                 density_plane_yin=[torch.zeros(1)])


def test_refusals_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library must not be loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (4, 4)):
        with pytest.raises(ValueError, match="at least 2 nodes"):
            geometry.box_lattice((0, 0, 0), (1, 1, 1), shape)
    with pytest.raises(ValueError, match="fewer than 2\\^31"):
        geometry.box_lattice((0, 0, 0), (1, 1, 1), (2048, 1024, 1024))
    with pytest.raises(ValueError, match="lo < hi"):
        geometry.box_lattice((0, 0, 0), (1, 0, 1), (4, 4, 4))
    radii = torch.tensor([0.5, 1.0, 2.0])
    with pytest.raises(ValueError, match="W >= 3"):
        geometry.panorama_lattice(4, 2, radii)
    with pytest.raises(ValueError, match="at least 2 nodes"):
        geometry.panorama_lattice(1, 8, radii)
    with pytest.raises(ValueError, match="at least 2 nodes"):
        geometry.panorama_lattice(4, 8, radii[:1])
    with pytest.raises(ValueError, match="fewer than 2\\^31"):
        geometry.panorama_lattice(32768, 65536, radii)
    for bad in ([0.5, 0.5, 2.0], [0.5, 0.4, 2.0], [0.0, 1.0, 2.0], [-1.0, 1.0, 2.0], [0.5, float("nan"), 2.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            geometry.panorama_lattice(4, 8, torch.tensor(bad))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.panorama_lattice(4, 8, radii)                      # good radii, but not on the device
    with pytest.raises(ValueError, match="r_near < r_far"):
        geometry.geometric_radii(2.0, 1.0, 4, device="cpu")
    assert np.array_equal(geometry.geometric_radii(0.5, 2.0, 3, device="cpu").numpy(), mref.geometric_radii(0.5, 2.0, 3))
    box = geometry.box_lattice((0, 0, 0), (1, 1, 1), (4, 5, 6))
    for level in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="must be finite"):
            geometry.extract_mesh(_stub(), box, level)
        with pytest.raises(ValueError, match="must be finite"):
            geometry.mesh_from_values(box, torch.zeros(120), level)
    with pytest.raises(NotImplementedError, match="plain exponential grid"):
        geometry.extract_mesh(_stub(interval_th=False), box, 1.0)
    with pytest.raises(TypeError, match="box_lattice or panorama_lattice"):
        geometry.extract_mesh(_stub(), (4, 5, 6), 1.0)
    with pytest.raises(ValueError, match="one per node"):
        geometry.mesh_from_values(box, torch.zeros(119), 0.0)


def test_refusals_of_the_device_and_the_workspace_cap(monkeypatch):
    box = geometry.box_lattice((0, 0, 0), (1, 1, 1), (4, 5, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.extract_mesh(_stub(), box, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.extract_mesh(_stub(interval_th=False), box, 1.0, normals=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.mesh_from_values(box, torch.zeros(120), 0.0)
    big = geometry.box_lattice((0, 0, 0), (1, 1, 1), (1024, 1024, 1024))       # 2^30 nodes: 6 GB of workspace and 4 GB of values
    with pytest.raises(ValueError, match="EGO_MESH_MAX_MB \\(4096; default 4096\\)"):
        geometry.extract_mesh(_stub(), big, 1.0)
    with pytest.raises(ValueError, match="EGO_MESH_MAX_MB"):
        geometry.mesh_from_values(big, torch.empty(2 ** 30, device="meta"), 1.0)
    monkeypatch.setenv("EGO_MESH_MAX_MB", "0.001")
    with pytest.raises(ValueError, match="EGO_MESH_MAX_MB \\(0; default 4096\\)"):
        geometry.extract_mesh(_stub(), box, 1.0)
    monkeypatch.setenv("EGO_MESH_MAX_MB", "lots")
    with pytest.raises(ValueError, match="number of megabytes"):
        geometry.extract_mesh(_stub(), box, 1.0)


def test_the_library_refuses_bad_lattices():
    lib = _lib.load()
    box = geometry.box_lattice((0, 0, 0), (1, 1, 1), (4, 5, 6))
    L = box.struct()
    assert lib.ego_mesh_workspace_bytes(L) >= 6 * 120
    L.n[1] = 1
    assert lib.ego_mesh_workspace_bytes(L) == -1
    assert lib.ego_mesh_count(L, 256, 0.0, 256, 1 << 20, 256, None) != 0 and b"at least 2 nodes" in lib.ego_last_error()
    L = box.struct()
    assert lib.ego_mesh_count(L, 256, float("nan"), 256, 1 << 20, 256, None) != 0 and b"finite" in lib.ego_last_error()
    assert lib.ego_mesh_count(L, 256, 0.0, 256, 16, 256, None) != 0 and b"smaller than" in lib.ego_last_error()
    assert lib.ego_mesh_emit(L, 256, 0.0, 256, 2 ** 31, 0, 256, 256, None) != 0 and b"2^31" in lib.ego_last_error()
    assert lib.ego_mesh_emit(L, None, 0.0, None, 0, 0, None, None, None) == 0          # nothing to emit: nothing queued
    assert lib.ego_point_gradient(None, None, 0, 0, None, None) != 0
    L.kind, L.H, L.W, L.n[2] = _lib.LATTICE_PANORAMA, 5, 2, 2
    assert lib.ego_mesh_workspace_bytes(L) == -1


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_and_bound():
    lib = _lib.load()
    for name, n_args in (("ego_mesh_field", 4), ("ego_mesh_workspace_bytes", 1), ("ego_mesh_count", 7), ("ego_mesh_emit", 9),
                         ("ego_point_gradient", 6)):
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib.os.path.dirname(_lib.os.path.abspath(_lib.__file__))), "include", "egonerf_hip.h")).read()
    assert "#define EGO_ABI_VERSION 17" in hdr and _lib.EXPECTED_ABI_VERSION == 17
    assert _lib.C.sizeof(_lib.LatticeStruct) == 112
