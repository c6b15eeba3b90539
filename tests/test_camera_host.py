"""CPU: the camera-path additions that need no GPU - exported symbols, argument validation of ego_camera_rays / ego_finish_frame
(refused before anything is queued), the numpy restatement of the finish arithmetic (tests/camera_ref.py) on hand-made values, the
restated pinhole directions against the reference's (tests/golden/camera_rays.npz), and evaluation_path's refusal of NDC rays."""
import ctypes as C

import numpy as np
import pytest

from egonerf_amd import _lib
from tests import camera_ref as ref

BADARG = -1


def test_library_exports_the_camera_symbols_and_abi_stays_17():
    lib = _lib.load()
    assert lib.ego_abi_version() == 17
    for name in ("ego_camera_rays", "ego_finish_frame"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and name in _lib.header_symbols()
    import egonerf_amd.renderer as r
    for name in ("camera_rays", "finish_frame", "FrameRenderer", "evaluation_path"):
        assert callable(getattr(r, name))


def _rays(lib, model=_lib.CAM_PINHOLE, H=4, W=6, fx=3.0, fy=3.0, first=0, count=0, c2w=None, rays=None):
    return lib.ego_camera_rays(model, H, W, fx, fy, W / 2, H / 2, 0, c2w, first, count, rays, None)


def test_camera_rays_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert _rays(lib) == 0                                                    # count == 0: a no-op, no pointer is looked at
    assert _rays(lib, model=_lib.CAM_ERP, fx=0.0, fy=0.0) == 0                # ERP needs no focal length
    assert _rays(lib, model=7) == BADARG
    assert _rays(lib, H=0) == BADARG and _rays(lib, W=-3) == BADARG
    assert _rays(lib, fx=0.0) == BADARG and _rays(lib, fy=0.0) == BADARG      # focal missing (the Python layer passes 0 for None)
    assert _rays(lib, fx=float("nan")) == BADARG and _rays(lib, fy=float("inf")) == BADARG
    assert b"focal" in lib.ego_last_error()
    assert _rays(lib, first=-1) == BADARG
    assert _rays(lib, first=20, count=5) == BADARG                            # first + count > H W
    assert _rays(lib, first=25) == BADARG
    assert _rays(lib, first=0, count=1 << 40) == BADARG
    assert b"window" in lib.ego_last_error()
    assert _rays(lib, first=24, count=0) == 0
    assert _rays(lib, count=4) == BADARG                                      # null pose / rays with work to do


def test_finish_frame_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    f = lambda first=0, count=0, H=4, W=6, mi=0.1, den=14.9, pal=None, sbs=0: lib.ego_finish_frame(None, None, first, count, H, W, mi, den, pal, sbs,
                                                                                                     None, None, None)
    assert f() == 0
    assert f(H=0) == BADARG and f(W=0) == BADARG
    assert f(first=20, count=5) == BADARG and f(first=-2) == BADARG
    assert f(den=0.0) == BADARG and f(mi=float("nan")) == BADARG
    assert f(sbs=1) == BADARG                                                 # side by side needs a palette
    assert f(count=3) == BADARG                                               # null buffers with work to do


def test_python_layer_checks_its_arguments():
    from egonerf_amd.camera import _camera_args, depth_range
    assert _camera_args(10, 20, "pinhole", None, None) == (_lib.CAM_PINHOLE, 0.0, 0.0, 10.0, 5.0)     # focal missing -> 0 -> EGO_E_BADARG
    assert _camera_args(10, 20, "pinhole_blender", 7, (1, 2)) == (_lib.CAM_PINHOLE_BLENDER, 7.0, 7.0, 1.0, 2.0)
    assert _camera_args(10, 20, "erp", None, None)[0] == _lib.CAM_ERP
    with pytest.raises(ValueError):
        _camera_args(10, 20, "fisheye", None, None)
    mi, den = depth_range([0.1, 15.0])
    assert (mi, den) == ref.depth_range([0.1, 15.0]) and mi.dtype == np.float32 and den == np.float32(15.0 - 0.1 + 1e-8)


def _exact_colour(v):
    """trunc(float32(clamp(v) * 255)): the float64 product of a float32 and 255 is exact, so one rounding to float32 follows it."""
    c = min(max(float(np.float32(v)), 0.0), 1.0)
    return int(np.float32(c * 255.0))


def test_finish_restatement_on_hand_made_colours():
    vals = [0.0, 1.0, 0.5, -0.25, 1.75, 0.999999, 1e-9]
    expect = [0, 255, 127, 0, 255, 254, 0]                                    # 0.5 * 255 = 127.5 truncates to 127
    for k in (1, 2, 3, 85, 127, 128, 200, 254, 255):                          # k / 255 and its float32 neighbours
        v = np.float32(k / 255.0)
        for w in (np.nextafter(v, np.float32(-1)), v, np.nextafter(v, np.float32(2))):
            vals.append(float(w))
            expect.append(_exact_colour(w))
    rgb = np.asarray(vals, np.float32).reshape(-1, 1).repeat(3, 1)
    rgb8, _, _ = ref.finish_ref(rgb, np.zeros(len(vals), np.float32), [0.0, 1.0])
    assert rgb8.dtype == np.uint8 and rgb8[:, 0].tolist() == expect
    # below k / 255 the byte is k - 1 or k, never k + 1; at or above it, k (or k - 1 where the product rounds down)
    assert all(abs(e - round(v * 255)) <= 1 for e, v in zip(expect, np.clip(vals, 0, 1)))


def test_finish_restatement_on_hand_made_depths():
    nf = [0.1, 15.0]
    mi, den = ref.depth_range(nf)
    d = np.asarray([0.1, 15.0, np.nan, 0.0, 0.05, 20.0, 1e30, np.inf, -np.inf, 7.55], np.float32)
    _, idx8, pal = ref.finish_ref(np.zeros((d.size, 3), np.float32), d, nf, palette=np.arange(768).reshape(256, 3) % 251)
    step = lambda x: int(np.float32(255.0 * float(np.float32(float(np.float32(x) - mi) / float(den)))))   # exact products, one rounding each
    assert idx8[0] == 0                                                       # depth == near
    assert idx8[1] == step(15.0) and idx8[1] in (254, 255)                    # depth == far: (far - near) / (far - near + 1e-8)
    assert idx8[2] == 0 and idx8[3] == 0 and idx8[4] == 0                     # NaN -> 0 -> below near; below near saturates to 0
    assert idx8[5] == 255 and idx8[6] == 255 and idx8[7] == 255               # above far saturates to 255 (numpy on x86 would wrap)
    assert idx8[8] == 0
    assert idx8[9] == step(7.55) == 127
    assert np.array_equal(pal, (np.arange(768).reshape(256, 3) % 251).astype(np.uint8)[idx8])


def test_restated_pinhole_directions_are_the_references_bits(golden):
    fx = golden("camera_rays")
    for case in ("small", "big"):
        H, W, focal = int(fx[f"{case}/H"]), int(fx[f"{case}/W"]), fx[f"{case}/focal"]
        center = None if np.isnan(fx[f"{case}/center"]).any() else fx[f"{case}/center"]
        for model in ("pinhole", "pinhole_blender"):
            d = ref.pinhole_dirs(H, W, focal, center, model == "pinhole_blender", fx[f"{case}/index"])
            assert d.dtype == np.float32 and np.array_equal(d.view(np.uint32), fx[f"{case}/dirs/{model}"].view(np.uint32))


def test_evaluation_path_refuses_ndc_rays():
    from egonerf_amd.renderer import evaluation_path
    with pytest.raises(NotImplementedError):
        evaluation_path(None, None, [], ndc_ray=True)
