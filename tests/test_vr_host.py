"""CPU: stereo panoramas and supersampled frames, the parts that need no GPU - the two exported symbols, the arguments
ego_camera_rays_ex / ego_resolve_frame refuse before anything is queued, FrameRenderer's argument checks (made before the model is
looked at) and the product shapes of stereo x side_by_side x palette."""
import numpy as np
import pytest

from egonerf_amd import _lib
from egonerf_amd import camera as cam

BADARG = -1


def test_library_exports_the_vr_symbols_and_abi_stays_17():
    lib = _lib.load()
    assert lib.ego_abi_version() == 17
    for name in ("ego_camera_rays_ex", "ego_resolve_frame"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and name in _lib.header_symbols()
    assert (_lib.EYE_CENTRE, _lib.EYE_LEFT, _lib.EYE_RIGHT) == (0, 1, 2)


def _rays(lib, model=_lib.CAM_ERP, H=8, W=16, fx=3.0, fy=3.0, first=0, count=0, eye=0, half_ipd=0.0, ss=1, c2w=None, rays=None):
    return lib.ego_camera_rays_ex(model, H, W, fx, fy, W / 2, H / 2, 1, c2w, first, count, eye, half_ipd, ss, rays, None)


def test_camera_rays_ex_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert _rays(lib) == 0                                                    # count == 0: a no-op
    assert _rays(lib, ss=2) == 0 and _rays(lib, ss=4) == 0 and _rays(lib, eye=2, half_ipd=0.065) == 0
    assert _rays(lib, ss=0) == BADARG and _rays(lib, ss=5) == BADARG and _rays(lib, ss=-1) == BADARG
    assert b"ss" in lib.ego_last_error()
    assert _rays(lib, ss=3) == BADARG                                         # 8 x 16 is not divisible by 3
    assert _rays(lib, H=9, W=16, ss=3) == BADARG and _rays(lib, H=9, W=15, ss=3) == 0
    assert _rays(lib, eye=3) == BADARG and _rays(lib, eye=-1) == BADARG
    for model in (_lib.CAM_PINHOLE, _lib.CAM_PINHOLE_BLENDER):                # the eyes exist for the panorama only
        assert _rays(lib, model=model) == 0
        assert _rays(lib, model=model, eye=1) == BADARG and _rays(lib, model=model, eye=2, half_ipd=0.1) == BADARG
    assert _rays(lib, eye=1, half_ipd=-0.1) == BADARG and _rays(lib, half_ipd=float("nan")) == BADARG
    assert _rays(lib, half_ipd=float("inf")) == BADARG
    # the window addresses OUTPUT pixels: 4 x 8 = 32 of them at ss = 2
    assert _rays(lib, ss=2, first=32) == 0 and _rays(lib, ss=2, first=33) == BADARG
    assert _rays(lib, ss=2, first=30, count=3) == BADARG and _rays(lib, first=-1) == BADARG
    assert b"window" in lib.ego_last_error()
    assert _rays(lib, model=_lib.CAM_PINHOLE, fx=0.0) == BADARG and _rays(lib, model=7) == BADARG
    assert _rays(lib, ss=2, count=4) == BADARG                                # null pose / rays with work to do


def test_resolve_frame_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    f = lambda first=0, count=0, H=4, W=8, ss=2, mi=0.1, den=14.9, pal=None, sbs=0: lib.ego_resolve_frame(
        None, None, first, count, H, W, ss, mi, den, pal, sbs, None, None, None)
    assert f() == 0 and f(ss=1) == 0 and f(ss=4) == 0 and f(ss=3) == 0       # H, W are the output frame's: nothing to divide
    assert f(ss=0) == BADARG and f(ss=5) == BADARG
    assert f(H=0) == BADARG and f(W=0) == BADARG
    assert f(first=30, count=3) == BADARG and f(first=-2) == BADARG
    assert f(den=0.0) == BADARG and f(mi=float("nan")) == BADARG
    assert f(sbs=1) == BADARG
    assert f(count=3) == BADARG


def test_python_layer_checks_eye_ipd_and_supersample():
    for bad in (0, 5, -1, 2.5):
        with pytest.raises(ValueError, match="supersample"):
            cam._supersample(bad)
    assert [cam._supersample(s) for s in (1, 2, 3, 4)] == [1, 2, 3, 4]
    with pytest.raises(ValueError, match="eye"):
        cam.camera_rays(8, 16, np.eye(4), eye="middle")
    with pytest.raises(ValueError, match="supersample"):
        cam.camera_rays(8, 16, np.eye(4), supersample=5)
    with pytest.raises(ValueError, match="ipd"):
        cam.camera_rays(8, 16, np.eye(4), eye="left", ipd=-1.0)
    assert cam._fine((_lib.CAM_PINHOLE, 7.0, 6.0, 8.0, 4.0), 3) == (_lib.CAM_PINHOLE, 21.0, 18.0, 24.0, 12.0)


def test_frame_renderer_refuses_stereo_it_cannot_render():
    """Checked before the model is touched: None stands in for it."""
    for camera in ("pinhole", "pinhole_blender"):
        with pytest.raises(ValueError, match="erp"):
            cam.FrameRenderer(None, 8, 16, camera=camera, focal=10.0, stereo="top_bottom", ipd=0.065)
    with pytest.raises(ValueError, match="ipd"):
        cam.FrameRenderer(None, 8, 16, stereo="top_bottom")
    with pytest.raises(ValueError, match="ipd"):
        cam.FrameRenderer(None, 8, 16, stereo="top_bottom", ipd=0.0)
    with pytest.raises(ValueError, match="stereo"):
        cam.FrameRenderer(None, 8, 16, stereo="left_right", ipd=0.065)
    for bad in (0, 5, -2):
        with pytest.raises(ValueError, match="supersample"):
            cam.FrameRenderer(None, 8, 16, supersample=bad)


@pytest.mark.parametrize("stereo", [None, "top_bottom"])
@pytest.mark.parametrize("side_by_side,with_palette", [(False, False), (False, True), (True, True)])   # side by side needs a palette
def test_product_shapes(stereo, side_by_side, with_palette):
    H, W = 8, 16
    shapes = cam.frame_shapes(H, W, with_palette, side_by_side, stereo)
    h = 2 * H if stereo else H
    if side_by_side:
        assert shapes == [(h, 2 * W, 3)]
    elif with_palette:
        assert shapes == [(h, W, 3), (h, W, 3)]
    else:
        assert shapes == [(h, W, 3), (h, W)]
