"""The stage-backward entry points (csrc/ego_stage_grad.hip) refuse null or invalid arguments with EGO_E_BADARG and a message, before
any device work: no GPU needed."""
import ctypes

from egonerf_amd import _lib


def test_stage_backward_argument_validation_needs_no_gpu():
    lib = _lib.load()
    sc = _lib.Scene()   # no tables, no weights
    g = _lib.VmGrad()
    checks = [
        (lambda: lib.ego_density_feature_backward_workspace_bytes(None, 16, 0), b"density_feature_backward"),
        (lambda: lib.ego_density_feature_backward_workspace_bytes(sc, 16, 0), b"density field"),
        (lambda: lib.ego_density_feature_backward(sc, None, 16, 0, None, ctypes.byref(g), None, 0, None), b"density_feature_backward"),
        (lambda: lib.ego_app_feature_backward_workspace_bytes(sc, -1), b"app_feature_backward"),
        (lambda: lib.ego_app_feature_backward(sc, None, 16, None, ctypes.byref(g), None, 160, None, 0, None), b"app_feature_backward"),
        (lambda: lib.ego_mlp_fea_backward_workspace_bytes(sc, 16), b"mlp_fea_backward"),
        (lambda: lib.ego_mlp_fea_backward(sc, None, None, 16, None, None, None, None, 0, None, 0, None, 0, None, 0, None), b"mlp_fea_backward"),
        (lambda: lib.ego_sh_render_backward(None, None, 16, None, None, None, None), b"sh_render_backward"),
        (lambda: lib.ego_sh_render_backward(None, None, -1, None, None, None, None), b"sh_render_backward"),
        (lambda: lib.ego_feature2density_backward(None, None, 16, None, None, None), b"feature2density_backward"),
        (lambda: lib.ego_raw2alpha_backward(None, None, None, 4, 8, None, None, None, None, None, None), b"raw2alpha_backward"),
        (lambda: lib.ego_raw2alpha_backward(None, None, None, 4, 0, None, None, None, None, None, None), b"raw2alpha_backward"),
    ]
    for call, what in checks:
        assert call() == -1
        assert what in lib.ego_last_error(), lib.ego_last_error()
