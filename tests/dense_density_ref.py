"""float64 reference of the dense density route (csrc/ego_dense.hip, k_march_density's dense form): the baked node grid, its trilinear
evaluation, and the factored formula it must reproduce (EgoNeRF.py:291-347), all in numpy from the reference's matMode / vecMode.

Tables are the 12 reference-shaped arrays of one field in field_tables' order (plane_yin[0..2], line_yin[0..2], plane_yang[0..2],
line_yang[0..2]): planes (1, C, res[m1], res[m0]), lines (1, C, res[vecMode], 1); res = (N_r, N_theta, N_phi)."""
import numpy as np

MAT_MODE = [[0, 1], [0, 2], [1, 2]]   # EgoNeRF.py:30-33: plane i spans (x axis, y axis)
VEC_MODE = [2, 1, 0]                  # ... and line i this axis


def _tables64(tables, g):
    planes = [np.asarray(tables[6 * g + i], np.float64)[0] for i in range(3)]      # [C][H][W]
    lines = [np.asarray(tables[6 * g + 3 + i], np.float64)[0, :, :, 0] for i in range(3)]   # [C][L]
    return planes, lines


def bake(tables, res):
    """-> (G, A): G [2][N_phi][N_theta][N_r][4] float64 = (G_0, G_1, G_2, 0) with G_i = sum_c plane_i,c[node] * line_i,c[node], and
    A [2][N_phi][N_theta][N_r][3] = sum_c |plane_i,c[node] * line_i,c[node]| (what the fp32 summation bound scales with)."""
    n = [int(v) for v in res]
    idx = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")   # [phi][theta][r] index arrays ...
    ax = {0: idx[2], 1: idx[1], 2: idx[0]}                                                # ... per axis 0 r, 1 theta, 2 phi
    G = np.zeros((2, n[2], n[1], n[0], 4))
    A = np.zeros((2, n[2], n[1], n[0], 3))
    for g in range(2):
        planes, lines = _tables64(tables, g)
        for i in range(3):
            m0, m1 = MAT_MODE[i]
            prod = planes[i][:, ax[m1], ax[m0]] * lines[i][:, ax[VEC_MODE[i]]]   # [C][phi][theta][r]
            G[g, ..., i] = prod.sum(0)
            A[g, ..., i] = np.abs(prod).sum(0)
    return G, A


def lin_taps(x, n):
    """F.grid_sample's taps along one axis of n nodes (align_corners=True, zero padding): clamped indices, weights 0 out of range."""
    ix = (np.asarray(x, np.float64) + 1.0) * (0.5 * (n - 1))
    fl = np.floor(ix)
    f = ix - fl
    i0, i1 = fl.astype(np.int64), fl.astype(np.int64) + 1
    w0 = np.where((i0 >= 0) & (i0 < n), 1.0 - f, 0.0)
    w1 = np.where((i1 >= 0) & (i1 < n), f, 0.0)
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), w0, w1


def factored_feature(tables, res, pts, yang):
    """sum_i relu(sum_c bilerp(plane_i,c) * lerp(line_i,c)) at normalised points pts [M][3] = (r, theta, phi) of grid yang [M] (0 | 1)."""
    pts, yang = np.asarray(pts, np.float64), np.asarray(yang).astype(bool)
    out = np.zeros(pts.shape[0])
    taps = [lin_taps(pts[:, a], int(res[a])) for a in range(3)]
    for g in range(2):
        planes, lines = _tables64(tables, g)
        feat = np.zeros(pts.shape[0])
        for i in range(3):
            m0, m1 = MAT_MODE[i]
            x0, x1, wx0, wx1 = taps[m0]
            y0, y1, wy0, wy1 = taps[m1]
            l0, l1, wl0, wl1 = taps[VEC_MODE[i]]
            P = (planes[i][:, y0, x0] * (wy0 * wx0) + planes[i][:, y0, x1] * (wy0 * wx1) + planes[i][:, y1, x0] * (wy1 * wx0)
                 + planes[i][:, y1, x1] * (wy1 * wx1))
            L = lines[i][:, l0] * wl0 + lines[i][:, l1] * wl1
            feat += np.maximum((P * L).sum(0), 0.0)
        out = np.where(yang == bool(g), feat, out)
    return out


def dense_feature(G, res, pts, yang):
    """sum_i relu(trilerp(G_i)) with the same taps: interpolation along r, then theta, then phi."""
    pts, g = np.asarray(pts, np.float64), np.asarray(yang).astype(np.int64)
    r0, r1, wr0, wr1 = lin_taps(pts[:, 0], int(res[0]))
    t0, t1, wt0, wt1 = lin_taps(pts[:, 1], int(res[1]))
    p0, p1, wp0, wp1 = lin_taps(pts[:, 2], int(res[2]))
    W = lambda w: w[:, None]
    along_r = lambda p, t: G[g, p, t, r0, :3] * W(wr0) + G[g, p, t, r1, :3] * W(wr1)
    u0 = along_r(p0, t0) * W(wt0) + along_r(p0, t1) * W(wt1)
    u1 = along_r(p1, t0) * W(wt0) + along_r(p1, t1) * W(wt1)
    return np.maximum(u0 * W(wp0) + u1 * W(wp1), 0.0).sum(-1)


def random_tables(res, seed, n_comp=16, scale=0.6):
    """12 random reference-shaped tables of a field at resolution res (field_tables' order)."""
    rng = np.random.default_rng(seed)
    out = []
    for _g in range(2):
        out += [(scale * rng.standard_normal((1, n_comp, res[MAT_MODE[i][1]], res[MAT_MODE[i][0]]))).astype(np.float32) for i in range(3)]
        out += [(scale * rng.standard_normal((1, n_comp, res[VEC_MODE[i]], 1))).astype(np.float32) for i in range(3)]
    return out


def probe_points(res, seed, n=600):
    """Normalised points [M][3] and grids [M]: random ones inside, on lattice planes (every axis), on the grid's faces (+-1) and
    outside [-1, 1], where taps are zero-padded (one and both taps of an axis out of range)."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.0, 1.0, (n, 3))
    lattice = rng.uniform(-1.0, 1.0, (n // 3, 3))
    for k in range(lattice.shape[0]):
        a = k % 3
        lattice[k, a] = 2.0 * rng.integers(0, res[a]) / (res[a] - 1) - 1.0
    faces = rng.uniform(-1.0, 1.0, (n // 3, 3))
    for k in range(faces.shape[0]):
        faces[k, k % 3] = -1.0 if (k // 3) % 2 else 1.0
    outside = rng.uniform(-1.0, 1.0, (n // 3, 3))
    for k in range(outside.shape[0]):
        a = k % 3
        step = 2.0 / (res[a] - 1)
        outside[k, a] = [1.0 + 0.4 * step, -1.0 - 0.4 * step, 1.0 + 1.7 * step, -1.0 - 2.5 * step][(k // 3) % 4]
    corners = np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
    pts = np.concatenate([pts, lattice, faces, outside, corners])
    return pts, (np.arange(pts.shape[0]) % 2)
