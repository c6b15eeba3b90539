"""float64 restatement of the dense appearance route (csrc/ego_dense.hip: ego_bake_app_dense; csrc/ego_shade.hip: gather_app_dense): the
baked node grid of the 27 appearance features, its trilinear evaluation, and the factored formula it must reproduce
(EgoNeRF.py:349-413), all in numpy from the reference's matMode / vecMode.

Tables are the 12 reference-shaped arrays of the appearance field in field_tables' order (plane_yin[0..2], line_yin[0..2],
plane_yang[0..2], line_yang[0..2]): planes (1, 48, res[m1], res[m0]), lines (1, 48, res[vecMode], 1); res = (N_r, N_theta, N_phi);
basis = (basis_mat_yin.weight, basis_mat_yang.weight), each [27][144] with column k = 48 i + c (plane-major).

Node layout (one node = 32 floats = 128 bytes, [grid][N_phi][N_theta][N_r][32], r fastest): eight quads of four floats; quad 2 q + h
holds slots 4 q .. 4 q + 3 of lane half h, and slot s of half h is feature 2 s + h (14 + 13 features, the fe registers of
csrc/ego_tuned.h).  So feature f sits at float node_float(f); the five floats that hold no feature are exactly 0.

Rounding count of the bake: the 144 products plane * line are exact in float64 (24 x 24 significant bits); each feature is one chain
of 144 float64 fused multiply-adds, one rounding each, and ONE rounding to float32 at the end.  The reference below sums in extended
precision (64 significant bits: its own 144 roundings stay below one float64 rounding of the sum of magnitudes), so a baked value
differs from it by at most half a float32 ulp plus gamma(K_BAKE) * sum |basis * product| with K_BAKE = 144 + 1."""
import numpy as np

from tests.dense_density_ref import MAT_MODE, VEC_MODE, lin_taps

APP_DIM, N_COMP, NODE_FLOATS = 27, 48, 32
K_BAKE = 144 + 1


def gamma(k, u=2.0 ** -53):
    return k * u / (1.0 - k * u)


def node_float(f):
    """Float of a node that holds feature f."""
    s, h = f >> 1, f & 1
    return (2 * (s >> 2) + h) * 4 + (s & 3)


FEATURE_FLOATS = np.array([node_float(f) for f in range(APP_DIM)])
PAD_FLOATS = np.array(sorted(set(range(NODE_FLOATS)) - set(FEATURE_FLOATS.tolist())))


def pack_nodes(feat):
    """[..., 27] features -> [..., 32] node floats (padding 0)."""
    out = np.zeros(feat.shape[:-1] + (NODE_FLOATS,), feat.dtype)
    out[..., FEATURE_FLOATS] = feat
    return out


def unpack_nodes(nodes):
    """[..., 32] node floats -> [..., 27] features."""
    return nodes[..., FEATURE_FLOATS]


def _tables(tables, g, dtype):
    planes = [np.asarray(tables[6 * g + i], dtype)[0] for i in range(3)]              # [C][H][W]
    lines = [np.asarray(tables[6 * g + 3 + i], dtype)[0, :, :, 0] for i in range(3)]   # [C][L]
    return planes, lines


def bake(tables, basis, res):
    """-> (F, A): F [2][N_phi][N_theta][N_r][27] float64 = basis_g . concat_i(plane_i[node] * line_i[node]), summed in extended
    precision, and A = sum_k |basis[f][k] * product_k| (what the float64 running-error bound scales with)."""
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended-precision long double"
    n = [int(v) for v in res]
    idx = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")   # [phi][theta][r] index arrays ...
    ax = {0: idx[2], 1: idx[1], 2: idx[0]}                                                # ... per axis 0 r, 1 theta, 2 phi
    F = np.zeros((2, n[2], n[1], n[0], APP_DIM))
    A = np.zeros((2, n[2], n[1], n[0], APP_DIM))
    for g in range(2):
        planes, lines = _tables(tables, g, np.longdouble)
        prod = np.concatenate([planes[i][:, ax[MAT_MODE[i][1]], ax[MAT_MODE[i][0]]] * lines[i][:, ax[VEC_MODE[i]]] for i in range(3)])
        B = np.asarray(basis[g], np.longdouble)                                           # [27][144]
        for f in range(APP_DIM):
            terms = B[f][:, None, None, None] * prod                                      # [144][phi][theta][r]
            F[g, ..., f] = terms.sum(0).astype(np.float64)
            A[g, ..., f] = np.abs(terms).sum(0).astype(np.float64)
    return F, A


def factored_feature(tables, basis, res, pts, yang):
    """basis_g . concat_i(bilerp(plane_i) * lerp(line_i)) at normalised points pts [M][3] = (r, theta, phi) of grid yang [M] -> [M][27]."""
    pts, yang = np.asarray(pts, np.float64), np.asarray(yang).astype(bool)
    out = np.zeros((pts.shape[0], APP_DIM))
    taps = [lin_taps(pts[:, a], int(res[a])) for a in range(3)]
    for g in range(2):
        planes, lines = _tables(tables, g, np.float64)
        v = []
        for i in range(3):
            m0, m1 = MAT_MODE[i]
            x0, x1, wx0, wx1 = taps[m0]
            y0, y1, wy0, wy1 = taps[m1]
            l0, l1, wl0, wl1 = taps[VEC_MODE[i]]
            P = (planes[i][:, y0, x0] * (wy0 * wx0) + planes[i][:, y0, x1] * (wy0 * wx1) + planes[i][:, y1, x0] * (wy1 * wx0)
                 + planes[i][:, y1, x1] * (wy1 * wx1))
            L = lines[i][:, l0] * wl0 + lines[i][:, l1] * wl1
            v.append(P * L)
        feat = (np.asarray(basis[g], np.float64) @ np.concatenate(v)).T
        out = np.where((yang == bool(g))[:, None], feat, out)
    return out


def dense_feature(F, res, pts, yang):
    """trilerp(F) with the same taps: interpolation along r, then theta, then phi -> [M][27]."""
    pts, g = np.asarray(pts, np.float64), np.asarray(yang).astype(np.int64)
    r0, r1, wr0, wr1 = lin_taps(pts[:, 0], int(res[0]))
    t0, t1, wt0, wt1 = lin_taps(pts[:, 1], int(res[1]))
    p0, p1, wp0, wp1 = lin_taps(pts[:, 2], int(res[2]))
    W = lambda w: w[:, None]
    along_r = lambda p, t: F[g, p, t, r0] * W(wr0) + F[g, p, t, r1] * W(wr1)
    u0 = along_r(p0, t0) * W(wt0) + along_r(p0, t1) * W(wt1)
    u1 = along_r(p1, t0) * W(wt0) + along_r(p1, t1) * W(wt1)
    return u0 * W(wp0) + u1 * W(wp1)


def random_basis(seed, scale=0.3):
    rng = np.random.default_rng(seed)
    return [(scale * rng.standard_normal((APP_DIM, 3 * N_COMP))).astype(np.float32) for _g in range(2)]


def c7n_of(pts, yang):
    """The [M][7] normalised coordinates (yin triple, yang triple, flag) the stage entry points take."""
    pts, yang = np.asarray(pts, np.float32), np.asarray(yang).astype(np.float32)[:, None]
    return np.concatenate([pts * (1 - yang), pts * yang, yang], -1).astype(np.float32)
