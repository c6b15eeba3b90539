"""Camera paths: a trained model and a list of camera poses in, the 8-bit frames of a walk-through out.

Mirror of renderer.py:199-255 (evaluation_path) and of the tail of renderer.py:141-174 (evaluation): rays per pose (dataLoader/
ray_utils.py:24-113), render, clamp, `(rgb * 255).astype('uint8')`, depth -> 8-bit index -> colours (utils.py:14-27), `rgbd` side by
side.  The two ends run on the device (csrc/ego_camera.hip): `camera_rays` reads the pose from device memory and writes one chunk of
rays in place, `finish_frame` writes bytes - 3 to 6 per pixel instead of 16 of float32 - into device or mapped pinned host memory.
In between is the unchanged `EgoNeRF.forward(need_alpha=False)`: the bits are those of `volume_renderer` on the same rays.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

CAMERA_MODELS = {"erp": _lib.CAM_ERP, "pinhole": _lib.CAM_PINHOLE, "pinhole_blender": _lib.CAM_PINHOLE_BLENDER}
EYES = {"centre": _lib.EYE_CENTRE, "left": _lib.EYE_LEFT, "right": _lib.EYE_RIGHT}
MAX_SUPERSAMPLE = 4


def _supersample(s) -> int:
    if int(s) != s or not 1 <= int(s) <= MAX_SUPERSAMPLE:
        raise ValueError(f"supersample {s!r}: expected an integer in 1..{MAX_SUPERSAMPLE}")
    return int(s)


def _fine(cam, ss: int):
    """The camera of the s x s sub-pixel samples: focal length and centre scaled by s (the caller scales H and W)."""
    code, fx, fy, cx, cy = cam
    return code, fx * ss, fy * ss, cx * ss, cy * ss


def _queue_rays(cam, H: int, W: int, normalize: bool, pose: torch.Tensor, first: int, count: int, eye: int, half_ipd: float, ss: int,
                out: torch.Tensor) -> None:
    """count * ss^2 rays of OUTPUT pixels [first, first + count) of the H x W frame into `out`, on the current stream.  The centre eye
    at one sample per pixel is ego_camera_rays as before; everything else goes through ego_camera_rays_ex."""
    lib = _lib.load()
    if eye == _lib.EYE_CENTRE and ss == 1:
        code, fx, fy, cx, cy = cam
        _lib.check(lib.ego_camera_rays(code, H, W, fx, fy, cx, cy, int(normalize), pose.data_ptr(), first, count, out.data_ptr(),
                                       _lib.stream_handle()), "ego_camera_rays")
        return
    code, fx, fy, cx, cy = _fine(cam, ss)
    _lib.check(lib.ego_camera_rays_ex(code, H * ss, W * ss, fx, fy, cx, cy, int(normalize), pose.data_ptr(), first, count, eye, half_ipd, ss,
                                      out.data_ptr(), _lib.stream_handle()), "ego_camera_rays_ex")


def _camera_args(H: int, W: int, model: str, focal, center) -> Tuple[int, float, float, float, float]:
    """(EGO_CAM_*, fx, fy, cx, cy).  A pinhole camera without `focal` passes 0, which the library refuses (EGO_E_BADARG); the default
    centre is the reference's `[W / 2, H / 2]` (dataLoader/ray_utils.py:58)."""
    if model not in CAMERA_MODELS:
        raise ValueError(f"camera model {model!r}: expected one of {sorted(CAMERA_MODELS)}")
    code = CAMERA_MODELS[model]
    if code == _lib.CAM_ERP:
        return code, 0.0, 0.0, 0.0, 0.0
    if focal is None:
        fx = fy = 0.0
    elif np.ndim(focal) == 0:
        fx = fy = float(focal)
    else:
        fx, fy = float(focal[0]), float(focal[1])
    cx, cy = (W / 2, H / 2) if center is None else (float(center[0]), float(center[1]))
    return code, fx, fy, cx, cy


def _pose_on_device(c2w, device) -> torch.Tensor:
    """The first 12 floats ([3][4] row-major) of a pose as a contiguous float32 device tensor; a device tensor of that form is used
    as it is (no copy: the kernel follows later writes to it)."""
    if isinstance(c2w, torch.Tensor) and c2w.is_cuda:
        if c2w.dtype != torch.float32 or not c2w.is_contiguous() or c2w.numel() < 12:
            raise ValueError("camera_rays: a device pose must be a contiguous float32 tensor of at least [3][4]")
        return c2w
    host = np.ascontiguousarray(np.asarray(c2w.cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32).reshape(-1)[:12])
    if host.size < 12:
        raise ValueError("camera_rays: c2w must hold at least [3][4]")
    return torch.from_numpy(host).to(device)


def camera_rays(H: int, W: int, c2w, model: str = "erp", focal=None, center=None, normalize: bool = True, first: int = 0,
                count: Optional[int] = None, device="cuda", out: Optional[torch.Tensor] = None, eye: str = "centre", ipd: float = 0.0,
                supersample: int = 1) -> torch.Tensor:
    """[count, 6] rays (origin, direction) of pixels [first, first + count) - row-major - of an H x W camera, generated on the device.

    model: "erp" (get_ray_directions_360, dataLoader/ray_utils.py:24-40; `normalize` as the ERP datasets do, the rows are bit-equal to
    `erp_rays`), "pinhole" (get_ray_directions, :43-61) or "pinhole_blender" (get_ray_directions_blender, :64-82), each followed by
    get_rays (:85-113; pinhole directions are not normalised, as there).  focal: a number or (fx, fy), required for the pinhole models;
    center: (cx, cy), default (W / 2, H / 2).  c2w: a host array, or a [3][4] (or [4][4]) float32 DEVICE tensor, which is read by the
    kernel when it runs - a captured launch follows a pose that is overwritten between replays.  `out`: a [>= count, 6] float32 device
    buffer to write into (its first `count` rows are returned).

    eye: "centre", or "left" / "right" (model="erp" only): the rays of one eye of an omnidirectional-stereo panorama - every pixel's
    origin lies on the viewing circle of diameter `ipd` (scene units, the full distance between the eyes), `ipd / 2` to the left / right
    of its horizontal viewing direction; the directions are the centre eye's.  supersample = s in 1..4: s x s rays per pixel, [count s^2,
    6]: row p s^2 + a s + b is pixel (row s + a, col s + b) of the (s H) x (s W) camera with focal length and centre scaled by s, the
    order `finish_frame(supersample=s)` averages.  H, W, focal, center, first and count stay those of the OUTPUT frame."""
    cam = _camera_args(H, W, model, focal, center)
    if eye not in EYES:
        raise ValueError(f"eye {eye!r}: expected one of {sorted(EYES)}")
    ss = _supersample(supersample)
    if not float(ipd) >= 0.0:
        raise ValueError("camera_rays: ipd must be >= 0")
    count = H * W - first if count is None else count
    n = max(count, 0) * ss * ss
    if out is None:
        out = torch.empty(n, 6, device=device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 2 and out.shape[1] == 6 and out.shape[0] >= n):
        raise ValueError("camera_rays: `out` must be a contiguous float32 device tensor [>= count * supersample^2, 6]")
    with torch.cuda.device(out.device):
        pose = _pose_on_device(c2w, out.device)
        _queue_rays(cam, H, W, bool(normalize), pose, first, count, EYES[eye], float(ipd) / 2, ss, out)
    return out[:n]


def depth_range(near_far) -> Tuple[np.float32, np.float32]:
    """(mi, den) of visualize_depth_numpy (utils.py:23-24) as float32: numpy evaluates `x - mi` and `/ (ma - mi + 1e-8)` on a float32
    array with Python floats, i.e. with float32(mi) and float32 of the sum formed in double precision."""
    mi, ma = float(near_far[0]), float(near_far[1])
    return np.float32(mi), np.float32(ma - mi + 1e-8)


_GRAY: dict = {}


def gray_palette(device) -> torch.Tensor:
    """The default palette: a gray ramp, palette[i] = (i, i, i)."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _GRAY:
        _GRAY[key] = torch.arange(256, dtype=torch.uint8).view(256, 1).repeat(1, 3).contiguous().to(dev)
    return _GRAY[key]


def _palette_on_device(palette, device) -> Optional[torch.Tensor]:
    """None -> the gray ramp; False -> no palette (the depth product is the 8-bit index); else 256 x 3 uint8 (any shape of 768 bytes)."""
    if palette is None:
        return gray_palette(device)
    if palette is False:
        return None
    t = palette if isinstance(palette, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(palette))
    if t.dtype != torch.uint8 or t.numel() != 768:
        raise ValueError("palette must hold 256 x 3 uint8 values")
    return t.reshape(256, 3).contiguous().to(device)


def _shapes(H: int, W: int, with_palette: bool, side_by_side: bool) -> List[Tuple[int, ...]]:
    if side_by_side:
        return [(H, 2 * W, 3)]
    return [(H, W, 3), (H, W, 3) if with_palette else (H, W)]


def frame_shapes(H: int, W: int, with_palette: bool, side_by_side: bool, stereo: Optional[str] = None) -> List[Tuple[int, ...]]:
    """The shapes of a frame's products: one eye's images, or with stereo="top_bottom" the left eye's on top of the right eye's."""
    eyes = 1 if stereo is None else 2
    return [(eyes * s[0],) + tuple(s[1:]) for s in _shapes(H, W, with_palette, side_by_side)]


def _finish(rgb, depth, first, H, W, mi, den, palette, side_by_side, bufs, ss: int = 1, offsets=(0, 0)) -> None:
    """Queues the finish (ss == 1) or resolve-and-finish kernel for rgb.shape[0] / ss^2 pixels from `first` on of an H x W image that
    begins `offsets[k]` bytes into bufs[k] (the second eye of a stereo frame)."""
    lib = _lib.load()
    out = [b.data_ptr() + o for b, o in zip(bufs, offsets)] + [None]
    if ss == 1:
        _lib.check(lib.ego_finish_frame(rgb.data_ptr(), depth.data_ptr(), first, rgb.shape[0], H, W, float(mi), float(den), _lib.ptr(palette),
                                        int(bool(side_by_side)), out[0], out[1], _lib.stream_handle()), "ego_finish_frame")
    else:
        _lib.check(lib.ego_resolve_frame(rgb.data_ptr(), depth.data_ptr(), first, rgb.shape[0] // (ss * ss), H, W, ss, float(mi), float(den),
                                         _lib.ptr(palette), int(bool(side_by_side)), out[0], out[1], _lib.stream_handle()), "ego_resolve_frame")


@torch.no_grad()
def finish_frame(rgb: torch.Tensor, depth: torch.Tensor, near_far, palette=None, side_by_side: bool = False, out=None, supersample: int = 1):
    """The frame products of renderer.py:227-240: float32 device `rgb` [H, W, 3] (or [n, 3]) and `depth` [H, W] (or [n]) ->
    (rgb8, depth8) uint8, or the one `rgbd` image [H, 2 W, 3] with side_by_side=True (np.concatenate((rgb8, depth8), axis=1)).

    rgb8 = (clamp(rgb, 0, 1) * 255) truncated; depth8 = palette[(255 * ((nan_to_num(depth) - near) / (far - near + 1e-8)))
    truncated], float32 operation by operation as numpy evaluates utils.py:14-25.  An index outside [0, 256) SATURATES (the
    reference's cast wraps on x86: DESIGN.md 3.2).  palette: 256 x 3 uint8; None = a gray ramp; False = no palette, depth8 is the
    index image [H, W].  No colour table is embedded - to reproduce the reference's bytes pass OpenCV's:

        palette = cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET).reshape(256, 3)

    out: the tensor(s) to write into, of the returned shapes: device memory or PINNED host memory (the kernel writes mapped host
    memory directly; synchronise the stream before reading it).

    supersample = s in 2..4: `rgb` [H, W, s^2, 3] (or [n s^2, 3]) and `depth` [H, W, s^2] (or [n s^2]) hold s x s samples per pixel in
    `camera_rays(supersample=s)`'s order; clamp(rgb, 0, 1) and nan_to_num(depth) are summed per pixel in float32, in sample order,
    divided by float32(s^2) and then quantised as above, in one kernel."""
    if not (rgb.is_cuda and depth.is_cuda):
        raise ValueError("finish_frame: rgb and depth must be device tensors (the HIP path has no CPU fallback)")
    ss = _supersample(supersample)
    flat = rgb.dim() == 2
    if flat and rgb.shape[0] % (ss * ss):
        raise ValueError(f"finish_frame: {rgb.shape[0]} colours are not whole groups of {ss * ss} samples")
    H, W = (1, rgb.shape[0] // (ss * ss)) if flat else (rgb.shape[0], rgb.shape[1])
    rgb = rgb.reshape(-1, 3).contiguous().float()
    depth = depth.reshape(-1).contiguous().float()
    if depth.shape[0] != rgb.shape[0]:
        raise ValueError(f"finish_frame: {rgb.shape[0]} colours but {depth.shape[0]} depths")
    if rgb.shape[0] != H * W * ss * ss:
        raise ValueError(f"finish_frame: supersample={ss} needs rgb [H, W, {ss * ss}, 3] or [n * {ss * ss}, 3]")
    with torch.cuda.device(rgb.device):
        pal = _palette_on_device(palette, rgb.device)
        if side_by_side and pal is None:
            raise ValueError("finish_frame: the side-by-side layout needs a palette")
        shapes = _shapes(H, W, pal is not None, side_by_side)
        if out is None:
            bufs = [torch.empty(s, dtype=torch.uint8, device=rgb.device) for s in shapes]
        else:
            bufs = [out] if isinstance(out, torch.Tensor) else list(out)
            for b, s in zip(bufs, shapes):
                if b.dtype != torch.uint8 or b.numel() != int(np.prod(s)) or not b.is_contiguous() or not (b.is_cuda or b.is_pinned()):
                    raise ValueError(f"finish_frame: `out` must be contiguous uint8 of shape {s}, on the device or in pinned host memory")
            if len(bufs) != len(shapes):
                raise ValueError(f"finish_frame: `out` must hold {len(shapes)} tensor(s)")
        mi, den = depth_range(near_far)
        _finish(rgb, depth, 0, H, W, mi, den, pal, side_by_side, bufs, ss)
    if flat and out is None and not side_by_side:
        bufs = [b.view(s[1:]) for b, s in zip(bufs, shapes)]   # [n, 3] in, [n, 3] / [n] out
    return bufs[0] if side_by_side else tuple(bufs)


class FrameRenderer:
    """Frames of one camera from poses: `render(c2w)` -> device uint8 images, `render_to_host(c2w)` -> pinned numpy arrays,
    `render_path(c2ws)` -> a generator over a path that yields frame k - 1 while frame k renders.

    camera / focal / center / normalize: as `camera_rays`.  palette / side_by_side: as `finish_frame` - the products are
    (rgb8 [H, W, 3], depth8 [H, W, 3]), (rgb8, idx8 [H, W]) with palette=False, or the one `rgbd` image [H, 2 W, 3].  near_far: the depth
    range of the index (default: the model's).  render_kwargs go to `EgoNeRF.forward` (n_coarse, n_fine, exp_sampling, resampling, ...).

    Per chunk of `chunk` pixels: rays into ONE reused chunk buffer (no full-image ray tensor), `model(rays, need_alpha=False)`, the finish
    kernel into the frame's images.  The pose lives in a device buffer that every render overwrites first.

    graph=True captures the whole frame once (torch.cuda.graph, on a single stream: no side stream, no parallel branches) and replays
    it per pose; it needs exp_sampling=True (the other schedule inspects device values on the host).  The capture fixes shapes and the
    scene's tables: re-create the object after `upsample_volume_grid` or a change of the alpha mask (`updateAlphaMask`,
    `use_alpha_mask`), the rule GraphedTrainStep documents for shapes.  With the dense density route (`EgoNeRF.dense_density`) the capture
    embeds the baked node grids, which are snapshots: after the density tables changed, call `model.scene()` before the next replay - it
    bakes into the same buffers, which stay allocated while the model keeps its device and grid size - and re-create the object after
    switching the route on or off.

    stereo="top_bottom" (camera="erp", ipd > 0 in scene units): an omnidirectional-stereo panorama for a headset player - the left
    eye's image on top of the right eye's in ONE image, so every product doubles in height ([2 H, W, 3], [2 H, W], `rgbd` [2 H, 2 W, 3]).
    The two eyes are rendered one after the other from the one device pose (`camera_rays(eye=...)`); each is a whole image, so the
    kernels of the second eye get the same buffers at an offset.  supersample = s in 1..4: s x s rays per pixel, averaged before the
    bytes are formed (`finish_frame(supersample=s)`); a chunk is still `chunk` PIXELS, i.e. chunk s^2 rays per render call."""

    def __init__(self, model, H: int, W: int, camera: str = "erp", focal=None, center=None, chunk: int = 16384, palette=None,
                 side_by_side: bool = False, graph: bool = False, near_far=None, normalize: bool = True, stereo: Optional[str] = None,
                 ipd: float = 0.0, supersample: int = 1, **render_kwargs):
        self.model, self.H, self.W, self.chunk = model, int(H), int(W), int(chunk)
        if self.chunk < 1 or self.H < 1 or self.W < 1:
            raise ValueError("FrameRenderer: H, W and chunk must be positive")
        self.cam = _camera_args(self.H, self.W, camera, focal, center)
        self.ss = _supersample(supersample)
        if stereo not in (None, "top_bottom"):
            raise ValueError(f"FrameRenderer: stereo {stereo!r}: expected None or 'top_bottom'")
        if stereo is not None and self.cam[0] != _lib.CAM_ERP:
            raise ValueError("FrameRenderer: a stereo panorama needs camera='erp'")
        if stereo is not None and not float(ipd) > 0.0:
            raise ValueError("FrameRenderer: a stereo panorama needs ipd > 0 (the distance between the eyes, in scene units)")
        self.stereo, self.half_ipd = stereo, float(ipd) / 2
        self.eyes = (_lib.EYE_CENTRE,) if stereo is None else (_lib.EYE_LEFT, _lib.EYE_RIGHT)
        if self.cam[0] != _lib.CAM_ERP and (self.cam[1] == 0.0 or self.cam[2] == 0.0):
            raise ValueError("FrameRenderer: a pinhole camera needs `focal`")
        self.normalize, self.side_by_side = bool(normalize), bool(side_by_side)
        if render_kwargs.get("ndc_ray"):
            raise NotImplementedError("ndc_ray (EgoNeRF.forward raises it as well, EgoNeRF.py:503-504)")
        self.kw = dict(render_kwargs)
        p = next(model.parameters())
        if not p.is_cuda:
            raise ValueError("FrameRenderer: the model must live on a HIP device")
        self.device = p.device
        self.mi, self.den = depth_range(model.near_far if near_far is None else near_far)
        with torch.cuda.device(self.device):
            self.palette = _palette_on_device(palette, self.device)
            if self.side_by_side and self.palette is None:
                raise ValueError("FrameRenderer: the side-by-side layout needs a palette")
            self._eye_shapes = _shapes(self.H, self.W, self.palette is not None, self.side_by_side)   # one eye's images
            self.shapes = frame_shapes(self.H, self.W, self.palette is not None, self.side_by_side, stereo)
            self._pose = torch.zeros(12, device=self.device, dtype=torch.float32)
            self._rays = torch.empty(min(self.chunk, self.H * self.W) * self.ss ** 2, 6, device=self.device, dtype=torch.float32)
            self._graph, self._static = None, None
            if graph:
                self._capture()

    # ---- buffers: flat uint8, padded to whole 16-byte blocks so that ego_copy_out can move any of them as float4s -----------------
    def _alloc(self, pinned: bool) -> List[torch.Tensor]:
        sizes = [(int(np.prod(s)) + 15) // 16 * 16 for s in self.shapes]
        if pinned:
            return [torch.empty(n, dtype=torch.uint8, pin_memory=True) for n in sizes]
        return [torch.empty(n, dtype=torch.uint8, device=self.device) for n in sizes]

    def _views(self, bufs):
        v = [b[:int(np.prod(s))].view(s) for b, s in zip(bufs, self.shapes)]
        return v[0] if self.side_by_side else tuple(v)

    # ---- one frame ----------------------------------------------------------------------------------------------------------------
    def _set_pose(self, c2w) -> None:
        if isinstance(c2w, torch.Tensor) and c2w.is_cuda:
            self._pose.copy_(c2w.reshape(-1)[:12].to(torch.float32))
            return
        host = np.asarray(c2w.cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32).reshape(-1)
        if host.size < 12:
            raise ValueError("FrameRenderer: c2w must hold at least [3][4]")
        stage = torch.empty(12, dtype=torch.float32, pin_memory=True)   # the caching host allocator keeps it alive until the copy has run
        stage.copy_(torch.from_numpy(np.ascontiguousarray(host[:12])))
        self._pose.copy_(stage, non_blocking=True)

    def _queue_chunks(self, bufs) -> None:
        """rays -> render -> finish for every chunk of every eye's image, on the current stream, from the pose in self._pose into `bufs`."""
        n, s2 = self.H * self.W, self.ss ** 2
        for k, eye in enumerate(self.eyes):
            offsets = [k * int(np.prod(s)) for s in self._eye_shapes]   # the k-th whole image of each buffer
            for first in range(0, n, self.chunk):
                count = min(self.chunk, n - first)
                rays = self._rays[:count * s2]
                _queue_rays(self.cam, self.H, self.W, self.normalize, self._pose, first, count, eye, self.half_ipd, self.ss, rays)
                rgb, depth = self.model(rays, need_alpha=False, **self.kw)[:2]
                _finish(rgb, depth, first, self.H, self.W, self.mi, self.den, self.palette, self.side_by_side, bufs, self.ss, offsets)

    def _capture(self) -> None:
        self._static = self._alloc(pinned=False)
        with torch.no_grad():
            self._queue_chunks(self._static)   # eager once: the library's self-test, the scene and schedule caches, the allocator's blocks
            torch.cuda.synchronize(self.device)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._queue_chunks(self._static)

    def _frame_into(self, c2w, bufs) -> None:
        """Queues one frame whose products land in `bufs` (device, or - eager only - mapped pinned memory)."""
        self._set_pose(c2w)
        if self._graph is None:
            self._queue_chunks(bufs)
            return
        self._graph.replay()
        if bufs is not self._static:   # device -> mapped host memory by the small copy kernel (renderer._render_to_host's hand-over)
            n = len(bufs)
            src = (C.c_void_p * n)(*[b.data_ptr() for b in self._static])
            dst = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
            cnt = (C.c_int64 * n)(*[b.numel() // 4 for b in bufs])
            _lib.check(_lib.load().ego_copy_out(n, src, dst, cnt, _COPY_WORKGROUPS, _lib.stream_handle()), "ego_copy_out")

    @torch.no_grad()
    def render(self, c2w):
        """(rgb8, depth8 | idx8) - or rgbd - as device tensors of the current stream (not synchronised)."""
        with torch.cuda.device(self.device):
            if self._graph is not None:
                self._frame_into(c2w, self._static)
                out = [b.clone() for b in self._static]   # the static images are overwritten by the next replay
            else:
                out = self._alloc(pinned=False)
                self._frame_into(c2w, out)
        return self._views(out)

    @torch.no_grad()
    def render_to_host(self, c2w):
        """The same products as numpy views of pinned host memory, complete on return."""
        with torch.cuda.device(self.device):
            out = self._alloc(pinned=True)
            self._frame_into(c2w, out)
            torch.cuda.current_stream().synchronize()
        v = self._views(out)
        return v.numpy() if self.side_by_side else tuple(t.numpy() for t in v)

    @torch.no_grad()
    def render_path(self, c2ws: Iterable) -> Iterator:
        """Yields the products of every pose in order, as numpy views of pinned host memory, frame k - 1 while frame k renders.

        Two sets of pinned images alternate; one event per set marks its frame complete.  A yielded frame is valid until the NEXT
        BUT ONE is asked for - the set is handed to frame k + 1 when the consumer comes back for frame k: copy what must live longer.
        Leaving the generator early waits for the queued frame before the images are released."""
        with torch.cuda.device(self.device):   # (not held across a yield: the consumer keeps its own current device)
            sets = [self._alloc(pinned=True) for _ in range(2)]
        done = [torch.cuda.Event() for _ in range(2)]
        queued = 0

        def host(k):
            v = self._views(sets[k & 1])
            return v.numpy() if self.side_by_side else tuple(t.numpy() for t in v)

        try:
            for c2w in c2ws:
                with torch.cuda.device(self.device):
                    self._frame_into(c2w, sets[queued & 1])
                    done[queued & 1].record(torch.cuda.current_stream())
                queued += 1
                if queued >= 2:
                    done[queued & 1].synchronize()   # frame queued - 2, in the other set
                    yield host(queued - 2)
            if queued:
                done[(queued - 1) & 1].synchronize()
                yield host(queued - 1)
        finally:
            if queued:
                done[(queued - 1) & 1].synchronize()   # an early exit: nothing queued may still write the images freed here


_COPY_WORKGROUPS = 16   # of ego_copy_out per frame: 3 to 12 MB once per frame, not 8 MB per chunk under the next chunk's march


@torch.no_grad()
def evaluation_path(test_dataset, model, c2ws, renderer=None, savePath=None, N_vis=5, prtx='', N_samples=-1, white_bg=False,
                    ndc_ray=False, compute_extra_metrics=True, exp_sampling=False, device='cuda', **frame_kwargs) -> List[np.ndarray]:
    """renderer.py:199-255 with the reference's signature: renders every pose of `c2ws` and returns the list of `rgbd` frames
    ([H, 2 W, 3] uint8: colour | depth colours, renderer.py:239); with `savePath` writes `{prtx}NNN.png` and `rgbd/{prtx}NNN.png` (PIL).

    `img_wh` and `near_far` - and `focal` (and `center`, if it has one) for camera="pinhole" / "pinhole_blender" - come from
    `test_dataset`.  frame_kwargs go to FrameRenderer (camera, palette, chunk, graph, stereo, ipd, supersample, n_coarse, n_fine,
    resampling, ...); N_samples > 0 is n_coarse unless that is given.  With stereo="top_bottom" the frames and both PNGs are twice as
    tall: [2 H, 2 W, 3], the left eye's rows above the right eye's.  `renderer`: a FrameRenderer to use as it is; anything else (the reference passes its chunk-loop
    function here) is ignored.  The two mp4 files of renderer.py:242-243 are NOT written (imageio is not a dependency; a warning says
    so).  ndc_ray=True raises NotImplementedError as EgoNeRF.forward does; white_bg, N_vis and compute_extra_metrics are accepted and
    unused, as in the reference."""
    if ndc_ray:
        raise NotImplementedError("ndc_ray (EgoNeRF.forward raises it as well, EgoNeRF.py:503-504)")
    W, H = test_dataset.img_wh
    if isinstance(renderer, FrameRenderer):
        fr = renderer
        if not fr.side_by_side or (fr.H, fr.W) != (H, W):
            raise ValueError("evaluation_path: the FrameRenderer must be side_by_side=True and of the dataset's image size")
    else:
        kw = dict(frame_kwargs)
        camera = kw.pop("camera", "erp")
        if camera != "erp":
            kw.setdefault("focal", test_dataset.focal)
            kw.setdefault("center", getattr(test_dataset, "center", None))
        if N_samples > 0:
            kw.setdefault("n_coarse", N_samples)
        kw.setdefault("near_far", test_dataset.near_far)
        fr = FrameRenderer(model, H, W, camera=camera, side_by_side=True, exp_sampling=exp_sampling, **kw)
    if savePath is not None:
        os.makedirs(os.path.join(savePath, "rgbd"), exist_ok=True)
    frames: List[np.ndarray] = []
    for idx, rgbd in enumerate(fr.render_path(c2ws)):
        rgbd = rgbd.copy()   # the pinned image goes back to the renderer
        frames.append(rgbd)
        if savePath is not None:
            from PIL import Image
            Image.fromarray(rgbd[:, :W]).save(os.path.join(savePath, f"{prtx}{idx:03d}.png"))
            Image.fromarray(rgbd).save(os.path.join(savePath, "rgbd", f"{prtx}{idx:03d}.png"))
    if savePath is not None:
        warnings.warn(f"evaluation_path: {prtx}video.mp4 and {prtx}depthvideo.mp4 (renderer.py:242-243) are not written: "
                      "encode the PNGs with a tool of your choice")
    return frames
