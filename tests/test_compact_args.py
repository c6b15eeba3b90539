"""Host-side checks of the compact shading path (include/egonerf_hip.h: ego_render_forward_compacts, ego_render_shaded_samples): argument
validation and workspace sizing, no device work."""
import ctypes

from egonerf_amd import _lib


def _align64(v):
    return (v + 63) & ~63


def _tile_path_floats(N, a):
    """The workspace of the tile paths alone (distances, weights, colours, coordinates, tile flags), in floats."""
    S = (a.n_coarse + a.n_fine if a.use_coarse_sample else a.n_fine) if a.resampling else a.n_coarse
    o = 0
    for n in (N * a.n_coarse, N * a.n_coarse if a.resampling else 0, N * S if a.resampling else 0, N * S, N, N * S * 3, N * S * 4,
              (N * S // 32 + 1 + 3) // 4):
        o = _align64(o + n)
    return o, S


def test_workspace_holds_the_live_list():
    lib = _lib.load()
    a = _lib.RenderArgs()
    a.n_coarse = 128
    assert lib.ego_render_workspace_bytes(-1, ctypes.byref(a)) == -1
    assert lib.ego_render_workspace_bytes(16, None) == -1
    a.n_coarse = 1
    assert lib.ego_render_workspace_bytes(16, ctypes.byref(a)) == -1
    for N, nc, nf, rs in ((4096, 512, 0, 0), (16384, 128, 128, 1), (1000, 100, 0, 0), (1, 2, 0, 0)):
        a = _lib.RenderArgs()
        a.n_coarse, a.n_fine, a.resampling, a.use_coarse_sample = nc, nf, rs, 1
        tiles, S = _tile_path_floats(N, a)
        got = lib.ego_render_workspace_bytes(N, ctypes.byref(a))
        assert got >= 4 * tiles + 4 * N * S, (N, S, got, 4 * tiles)


def test_compacts_is_a_host_question():
    lib = _lib.load()
    assert lib.ego_render_forward_compacts(None, 4096, 256) == 0
    sc = _lib.Scene()   # app_dim 0 etc.: not the tuned shape -> today's kernels, whatever the mask and the threshold say
    sc.weight_thres = 1e-4
    assert lib.ego_render_forward_compacts(ctypes.byref(sc), 4096, 256) == 0


def test_shaded_samples_refuses_an_unknown_workspace():
    lib = _lib.load()
    a = _lib.RenderArgs()
    a.n_coarse = 64
    out = ctypes.c_int64(0)
    ws = ctypes.create_string_buffer(64)   # never handed to ego_render_forward: refused before any launch
    assert lib.ego_render_shaded_samples(16, ctypes.byref(a), ws, ctypes.byref(out), None) == -1
    assert b"no ego_render_forward" in lib.ego_last_error()
    assert lib.ego_render_shaded_samples(16, None, ws, ctypes.byref(out), None) == -1
    assert lib.ego_render_shaded_samples(0, ctypes.byref(a), ws, ctypes.byref(out), None) == -1
