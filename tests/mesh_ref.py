"""The restatement of the iso-surface extraction (csrc/ego_mesh.hip, include/egonerf_hip.h): lattices, marching tetrahedra on
the Kuhn decomposition, vertex and face order, winding - in numpy, positions in float32 (what the kernel must return bit for bit on a box
lattice) or float64 (what bounds it on a panorama lattice, whose directions pass through sinf / cosf).  This file is the executable
definition; the kernel matches it.  Also the topology checks both test files apply, analytic fields, and the oracle's sigma on a lattice.

`python -m tests.mesh_ref` measures the bounds below on the CPU."""
import collections
import itertools
import math

import numpy as np

BOX, PANORAMA = 0, 1
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))   # the six tetrahedra of a cell, in this order
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))                  # pairs of a tetrahedron's corners, low corner first


def parity(p) -> int:
    """0 for an even permutation, 1 for an odd one."""
    return sum(1 for a, b in itertools.combinations(range(len(p)), 2) if p[a] > p[b]) & 1


def tet_corners(t):
    """The corner bit triples (bit a = one step along axis a) of tetrahedron t: 000, e_p0, e_p0 + e_p1, 111."""
    p = PERMS[t]
    return (0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7)


def tet_case(mask):
    """Triangles of a tetrahedron whose corner c is inside where bit c of `mask` is set, as triples of TET_EDGES indices, wound so that
    (v1 - v0) x (v2 - v0) points to the outside when det[c1 - c0, c2 - c0, c3 - c0] > 0 (the caller swaps the last two otherwise)."""
    e = lambda a, b: TET_EDGES.index((min(a, b), max(a, b)))
    inside = [c for c in range(4) if mask >> c & 1]
    outside = [c for c in range(4) if not mask >> c & 1]
    if len(inside) in (0, 4):
        return []
    if len(inside) in (1, 3):
        i = (inside if len(inside) == 1 else outside)[0]
        j, k, l = [c for c in range(4) if c != i]
        if parity((i, j, k, l)):
            k, l = l, k
        return [(e(i, j), e(i, k), e(i, l))] if len(inside) == 1 else [(e(i, j), e(i, l), e(i, k))]
    (i, j), (k, l) = inside, outside
    if parity((i, j, k, l)):
        k, l = l, k
    return [(e(i, k), e(i, l), e(j, l)), (e(i, k), e(j, l), e(j, k))]


CASES = [tet_case(m) for m in range(16)]
POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


class Lattice(collections.namedtuple("Lattice", "kind n origin step radii H W c2w")):
    """A lattice as the kernel receives it: float32 numbers (origin, step [3]; radii [n0]; c2w [3,4]).  Axis 0 is fastest."""

    @property
    def wrap(self):
        return self.kind == PANORAMA

    @property
    def flip(self):   # the handedness of (axis 0, axis 1, axis 2): rows run down and columns run clockwise seen from above
        return int(self.kind == PANORAMA)

    @property
    def count(self):
        return int(self.n[0]) * int(self.n[1]) * int(self.n[2])


def box(lo, hi, shape):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    n = tuple(int(s) for s in shape)
    return Lattice(BOX, n, lo.astype(np.float32), ((hi - lo) / (np.asarray(n) - 1)).astype(np.float32), None, 0, 0, None)


def panorama(H, W, radii, c2w=None):
    c2w = np.concatenate([np.eye(3), np.zeros((3, 1))], 1) if c2w is None else c2w
    radii = np.asarray(radii, np.float32)
    return Lattice(PANORAMA, (len(radii), int(H), int(W)), None, None, radii, int(H), int(W), np.asarray(c2w, np.float32).reshape(3, 4))


def geometric_radii(r_near, r_far, n):
    return (float(r_near) * (float(r_far) / float(r_near)) ** (np.arange(n, dtype=np.float64) / (n - 1))).astype(np.float32)


def node_index(lat):
    m = np.arange(lat.count, dtype=np.int64)
    return m % lat.n[0], m // lat.n[0] % lat.n[1], m // (lat.n[0] * lat.n[1])


def erp_directions(H, W, row, col, c2w, dt):
    """erp_ray of csrc/ego_device.h with normalize = 1, operation by operation in `dt`; pi is the float32 constant in float32."""
    f = dt
    pi = f(np.float32(math.pi)) if dt is np.float32 else f(math.pi)
    i, j = col.astype(dt) + f(0.5), row.astype(dt) + f(0.5)
    phi = (f(1) - f(2) * i / f(W)) * pi
    theta = (f(1) - f(2) * j / f(H)) * pi / f(2)
    ct = np.cos(theta)
    d = [-ct * np.sin(phi), np.sin(theta), -ct * np.cos(phi)]
    nrm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    d = [c / nrm for c in d]
    m = c2w.astype(dt)
    return np.stack([(d[0] * m[r, 0] + d[1] * m[r, 1]) + d[2] * m[r, 2] for r in range(3)], -1), m[:, 3]


def positions(lat, dt=np.float32):
    """[count, 3] node positions in `dt`: origin + (float) i * step, or o + radii[k] * d; every operation rounded once."""
    i0, i1, i2 = node_index(lat)
    if lat.kind == BOX:
        return np.stack([lat.origin[a].astype(dt) + i.astype(dt) * lat.step[a].astype(dt) for a, i in enumerate((i0, i1, i2))], -1)
    d, o = erp_directions(lat.H, lat.W, i1, i2, lat.c2w, dt)
    return o[None, :] + lat.radii.astype(dt)[i0][:, None] * d


def neighbour(lat, bits):
    """(node id of the node `bits` away, whether it exists) for every node; axis 2 of a panorama lattice wraps."""
    i0, i1, i2 = node_index(lat)
    j0, j1, j2 = i0 + (bits & 1), i1 + (bits >> 1 & 1), i2 + (bits >> 2 & 1)
    ok = (j0 < lat.n[0]) & (j1 < lat.n[1])
    if lat.wrap:
        j2 = j2 % lat.n[2]
    else:
        ok &= j2 < lat.n[2]
    return np.where(ok, (j2 * lat.n[1] + j1) * lat.n[0] + j0, 0), ok


def classify(lat, values, level):
    """(inside [count] bool, flags [count] uint8: bit k = the owned edge k crosses, offsets [count] = exclusive scan of the flag counts)."""
    with np.errstate(invalid="ignore"):
        inside = np.asarray(values, np.float32).reshape(-1) >= np.float32(level)   # NaN is outside
    flags = np.zeros(lat.count, np.int64)
    for k in range(7):
        nb, ok = neighbour(lat, k + 1)
        flags |= (ok & (inside != inside[nb])).astype(np.int64) << k
    cnt = POPCOUNT8[flags]
    return inside, flags, np.cumsum(cnt) - cnt


def extract(lat, values, level, dt=np.float32):
    """(vertices [V,3] `dt`, faces [F,3] int32) of the surface value = level on `lat`."""
    values = np.asarray(values, np.float32).reshape(-1)
    assert values.shape[0] == lat.count
    inside, flags, off = classify(lat, values, level)
    pos = positions(lat, dt)
    V = int(POPCOUNT8[flags].sum())
    verts = np.zeros((V, 3), dt)
    lv = np.float32(level).astype(dt)
    for k in range(7):
        a = np.nonzero(flags >> k & 1)[0]
        b = neighbour(lat, k + 1)[0][a]
        fa, fb = values[a].astype(dt), values[b].astype(dt)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            t = (lv - fa) / (fb - fa)
        t = np.where(np.isfinite(t), np.clip(t, 0, 1), dt(0.5)).astype(dt)
        vid = off[a] + POPCOUNT8[flags[a] & ((1 << k) - 1)]
        verts[vid] = pos[a] + t[:, None] * (pos[b] - pos[a])
    cells = np.nonzero(neighbour(lat, 7)[1])[0]
    corner = [neighbour(lat, b)[0][cells] for b in range(8)]
    keys, tris = [], []
    for t in range(6):
        cb = tet_corners(t)
        mask = sum(inside[corner[cb[c]]].astype(np.int64) << c for c in range(4))
        swap = parity(PERMS[t]) ^ lat.flip
        for m in range(1, 15):
            sel = np.nonzero(mask == m)[0]
            for j, tri in enumerate(CASES[m]):
                ids = []
                for e in (tri if not swap else (tri[0], tri[2], tri[1])):
                    ca, cbb = cb[TET_EDGES[e][0]], cb[TET_EDGES[e][1]]
                    own, k = corner[ca][sel], (cbb ^ ca) - 1
                    ids.append(off[own] + POPCOUNT8[flags[own] & ((1 << k) - 1)])
                tris.append(np.stack(ids, -1))
                keys.append(np.stack([cells[sel], np.full(len(sel), t), np.full(len(sel), j)], -1))
    if not tris:
        return verts, np.zeros((0, 3), np.int32)
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return verts, tris[order].astype(np.int32)


# ---- topology and orientation --------------------------------------------------------------------------------------------------------
def topology(faces, n_vertices):
    """dict(V, E, F, chi, boundary: undirected edges in one face only, consistent: every edge in at most two faces and, where in two,
    traversed once in each direction)."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und, inv, cnt = np.unique(np.sort(d, 1), axis=0, return_inverse=True, return_counts=True)
    sign = np.where(d[:, 0] < d[:, 1], 1, -1)
    net = np.bincount(inv.reshape(-1), weights=sign, minlength=len(und))
    used = len(np.unique(f))
    consistent = bool((cnt <= 2).all() and (net[cnt == 2] == 0).all() and (d[:, 0] != d[:, 1]).all())
    return dict(V=used, E=len(und), F=len(f), chi=used - len(und) + len(f), boundary=und[cnt == 1], consistent=consistent,
                all_used=used == n_vertices)


def face_normals(vertices, faces):
    v = np.asarray(vertices, np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]), v[faces].mean(1)


def winding_agrees(vertices, faces, outward, tiny=1e-12):
    """Every non-degenerate face normal has a positive dot product with outward(centroid) [F,3] -> (all agree, faces judged)."""
    n, c = face_normals(vertices, faces)
    live = np.linalg.norm(n, axis=1) > tiny
    return bool(((n[live] * outward(c[live])).sum(1) > 0).all()), int(live.sum())


def vertex_nodes(lat, values, level):
    """[V,2] the two end nodes (owner, far) of every vertex's edge, in vertex order."""
    _, flags, off = classify(lat, values, level)
    out = np.zeros((int(POPCOUNT8[flags].sum()), 2), np.int64)
    for k in range(7):
        a = np.nonzero(flags >> k & 1)[0]
        out[off[a] + POPCOUNT8[flags[a] & ((1 << k) - 1)]] = np.stack([a, neighbour(lat, k + 1)[0][a]], -1)
    return out


# ---- analytic fields (positive inside, level 0) ------------------------------------------------------------------------------------
def sphere(c, R):
    c = np.asarray(c, np.float64)
    return (lambda p: R - np.linalg.norm(p - c, axis=-1)), (lambda p: (p - c) / np.linalg.norm(p - c, axis=-1, keepdims=True))


def torus(c, R, r):
    c = np.asarray(c, np.float64)

    def parts(p):
        q = p - c
        rho = np.hypot(q[..., 0], q[..., 1])
        return q, rho, np.sqrt((rho - R) ** 2 + q[..., 2] ** 2)

    def value(p):
        return r - parts(p)[2]

    def outward(p):
        q, rho, d = parts(p)
        return np.stack([(rho - R) * q[..., 0] / rho, (rho - R) * q[..., 1] / rho, q[..., 2]], -1) / d[..., None]
    return value, outward


# ---- the lattices and bounds of tests/test_hip_mesh.py --------------------------------------------------------------------------------
def skew_pose():
    """A rotation about a skew axis and a small offset, float32."""
    a = np.array([0.3, -0.5, 0.4])
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    return np.concatenate([R, np.array([[0.05], [-0.02], [0.03]])], 1).astype(np.float32)


def panorama_cases():
    return {"4x5x3": panorama(5, 3, geometric_radii(0.5, 2.0, 4), skew_pose()), "6x16x33": panorama(16, 33, geometric_radii(0.2, 9.0, 6), skew_pose())}


def random_values(lat, seed):
    return np.random.default_rng(seed).standard_normal(lat.count).astype(np.float32)


# Panorama vertices, kernel against the float64 restatement, absolute in the max norm: 4 x the float32 restatement's own worst distance
# from the float64 one over panorama_cases() with random_values(seed 1), level 0 (python -m tests.mesh_ref):
#   4x5x3 3.02e-7 (largest radius 2), 6x16x33 2.58e-6 (largest radius 9)
B_PANORAMA = {"4x5x3": 4 * 3.02e-7, "6x16x33": 4 * 2.58e-6}


# ---- sigma on a lattice, from the oracle ---------------------------------------------------------------------------------------------
FIELD_CASES = ("tiny", "odd_grid", "other_n_comp")
CHART_MARGIN, CENTRE_MARGIN, MOST_LEFT_OUT = 1e-5, 1e-6, 0.01


def field_lattices(oracle):
    """A 9x7x5 box reaching into both charts and a 5x8x16 panorama lattice around the oracle's centre; origins and steps offset and not
    commensurate with pi/4, so that no node sits on a chart boundary."""
    c = oracle.center.double().numpy()
    far = float(oracle.far_r)
    h = 0.35 * far
    lo = c + np.array([-0.83, -0.91, -0.77]) * h
    hi = c + np.array([0.89, 0.79, 0.93]) * h
    pose = skew_pose().astype(np.float64)
    pose[:, 3] = c + np.array([0.013, -0.007, 0.011]) * far
    return {"box": box(lo, hi, (9, 7, 5)), "panorama": panorama(8, 16, geometric_radii(0.04 * far, 0.6 * far, 5), pose)}


def oracle_sigma(oracle, lat):
    """(sigma [count] in the oracle's dtype at the float32 node positions, yang [count], keep [count]: nodes that are neither within
    CHART_MARGIN rad of a chart boundary nor within CENTRE_MARGIN of the centre, judged in float64)."""
    import torch
    x = torch.from_numpy(positions(lat, np.float32)).to(oracle.dtype)
    with torch.no_grad():
        c7 = oracle.from_cartesian(x)
        sigma = oracle.feature2density(oracle.density_feature(oracle.normalize_coord(c7, downsample=None)))
        keep = (oracle.yin_margin(x).abs() >= CHART_MARGIN) & ((x.double() - oracle.center.double()).norm(dim=-1) >= CENTRE_MARGIN)
    return sigma, c7[..., 6] != 0, keep


# ego_mesh_field against the float64 oracle, relative to max |sigma64| of the lattice: 4 x the float32 oracle's own worst distance from the
# float64 one on the same nodes over FIELD_CASES x field_lattices (python -m tests.mesh_ref); the oracle alone leaves out no node:
#   worst 2.40e-6 (odd_grid, box; 9.4e-7 to 2.3e-6 elsewhere); both charts occur on every lattice (145 of 315 and 205 of 640 nodes on yang)
B_FIELD = 4 * 2.40e-6


def measure_bounds():
    import torch
    from tests import ray_grad_ref as rg
    from tests.helpers import make_oracle
    for name, lat in panorama_cases().items():
        v = random_values(lat, 1)
        a, fa = extract(lat, v, 0.0, np.float32)
        b, fb = extract(lat, v, 0.0, np.float64)
        assert np.array_equal(fa, fb)
        print(f"panorama {name}: V {len(a)} F {len(fa)}  |f32 - f64| {np.abs(a.astype(np.float64) - b).max():.3e}  largest radius {lat.radii.max():.3g}")
    for case in FIELD_CASES:
        cfg, w, *_ = rg.case_inputs(case)
        o64, o32 = make_oracle(cfg, w, dtype=torch.float64), make_oracle(cfg, w)
        for name, lat in field_lattices(o64).items():
            s64, yang, keep = oracle_sigma(o64, lat)
            s32, yang32, _ = oracle_sigma(o32, lat)
            scale = float(s64.abs().max())
            err = float((s32.double() - s64)[keep & (yang == yang32)].abs().max()) / scale
            print(f"field {case:13s} {name:9s} nodes {lat.count}  yang {int(yang.sum())}  left out {int((~keep).sum())}  chart differs in float32 "
                  f"{int((yang != yang32).sum())}  max sigma {scale:.3e}  |f32 - f64| / max {err:.3e}")


if __name__ == "__main__":
    measure_bounds()
