"""Render driver: mirror of renderer.py:11-79 (volume_renderer) and the PSNR part of
renderer.py:82-196 (evaluation), plus the multi-GPU sharding of SURVEY 8(e).

Rays are independent, so N GPUs = N processes each rendering a contiguous block of rays with a
replicated (read-only) model; the only exchange is the 2-float [sum of squared error, pixel count]
all-reduce per image for PSNR and an optional gather of the tiles (torch.distributed: RCCL on GPUs,
gloo in the CPU tests).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch


def volume_renderer(rays, model, chunk=4096, n_coarse=-1, n_fine=0, ndc_ray=False, white_bg=True, is_train=False,
                    exp_sampling=False, device="cuda", empty_gpu_cache=False, pretrain_envmap=False, pivotal_sample_th=0.0,
                    resampling=False, use_coarse_sample=True, interval_th=False, jitter=None, u=None, keep_alpha=True):
    """renderer.py:11-79.  Returns (rgb [N,3], depth [N], bg|None, env|None, alpha [N,S(+1)]); numpy arrays
    when `empty_gpu_cache` (per-chunk D2H like the reference), torch tensors otherwise.  keep_alpha=False drops the
    per-sample alpha (2 GB for a 1024 x 2048 image at 256 samples; only the entropy loss reads it) and returns None there."""
    if pretrain_envmap:
        return model(rays_chunk=rays.to(device), pretrain_envmap=True)
    outs: List[Tuple] = []
    n_all = rays.shape[0]
    dev = torch.device(device)
    if empty_gpu_cache and dev.type == "cuda" and isinstance(rays, torch.Tensor):
        return _render_to_host(rays, model, chunk, dev, keep_alpha, jitter, u,
                               dict(is_train=is_train, white_bg=white_bg, ndc_ray=ndc_ray, n_coarse=n_coarse, n_fine=n_fine, exp_sampling=exp_sampling,
                                    pivotal_sample_th=pivotal_sample_th, resampling=resampling, use_coarse_sample=use_coarse_sample,
                                    interval_th=interval_th))
    if dev.type == "cuda" and isinstance(rays, torch.Tensor) and rays.device.type == "cpu" and 0 < rays.numel() * rays.element_size() <= _UPLOAD_BYTES:
        # a host ray list goes up ONCE through pinned memory instead of one blocking pageable copy per chunk (renderer.py:26 does the
        # latter: 6.1 M rays/s against 7.4 M resident at 4096 x 512, tools/pcie_inclusive.py); the chunks are then device slices
        stage = rays if rays.is_pinned() else torch.empty(rays.shape, dtype=rays.dtype, pin_memory=True).copy_(rays)
        rays = stage.to(dev, non_blocking=True)
    for lo in range(0, max(n_all, 1), chunk):  # an empty ray list still makes one (empty) call, so the outputs keep their shapes
        rays_chunk = rays[lo:lo + chunk].to(device)
        kw = dict(jitter=None if jitter is None else jitter[lo:lo + chunk], u=None if u is None else u[lo:lo + chunk])
        if not keep_alpha and getattr(model, "supports_need_alpha", False):
            kw["need_alpha"] = False  # this package's EgoNeRF: no [N,S] alpha buffer, and the march may stop at transmittance 0
        o = model(rays_chunk, is_train=is_train, white_bg=white_bg, ndc_ray=ndc_ray, n_coarse=n_coarse, n_fine=n_fine,
                  exp_sampling=exp_sampling, pivotal_sample_th=pivotal_sample_th, resampling=resampling,
                  use_coarse_sample=use_coarse_sample, interval_th=interval_th, **kw)
        if not keep_alpha:
            o = o[:4] + (None,)
        if empty_gpu_cache:
            o = tuple(None if t is None else t.cpu().numpy() for t in o)
        outs.append(o)
    cat = (lambda xs: np.concatenate(xs)) if empty_gpu_cache else (lambda xs: torch.cat(xs))
    col = lambda j: None if outs[0][j] is None else cat([o[j] for o in outs])
    return col(0), col(1), col(2), col(3), col(4)


_UPLOAD_BYTES = 256 << 20   # host ray lists up to this size go to the device in one pinned, asynchronous copy


def _render_to_host(rays, model, chunk, dev, keep_alpha, jitter, u, kw):
    """volume_renderer(..., empty_gpu_cache=True) - the reference's own call pattern (renderer.py:26, :39-53: every chunk's outputs leave
    the device, the [chunk, S] alpha included) - without its stalls.  The reference's `.cpu().numpy()` per chunk is a BLOCKING copy into
    pageable memory followed by one more copy of everything in np.concatenate (2.30 M rays/s at 4096 x 512 against 7.4 M resident,
    VERDICT r05 item 5).  Here every output is copied device -> host ONCE, asynchronously, on a side stream, straight into its rows of
    one pinned array per output (the returned numpy arrays are views of those: no concatenate), while the next chunk's kernels run; the
    ray list, if it lives on the host, goes up through a pinned buffer in one asynchronous copy instead of one pageable copy per chunk.
    Same kernels, same order per chunk: the values are bit-identical to the resident path."""
    n_all = rays.shape[0]
    main = torch.cuda.current_stream(dev)
    if rays.device.type == "cpu" and rays.numel() * rays.element_size() <= _UPLOAD_BYTES and n_all:
        stage = rays if rays.is_pinned() else torch.empty(rays.shape, dtype=rays.dtype, pin_memory=True).copy_(rays)
        rays = stage.to(dev, non_blocking=True)
        hold = stage   # the pinned source must outlive the copy: referenced until the final synchronisation
    side = _copy_stream(dev)
    host: List[Optional[torch.Tensor]] = [None] * 5
    # The runtime copies device -> pinned host with a blit KERNEL (`__amd_rocclr_copyBuffer`: 170 us for the 8 MB alpha of a chunk), and next
    # to it the following chunk's march - bound by the latency of its own gathers - took 260 us instead of 97 (tools/handover_timeline.sh;
    # stream priorities changed nothing).  So chunk k's copies wait for chunk k + 1's MARCH (ego_render_args.marched) and run under its
    # shade kernel, which is bound by instruction issue and has the memory system to spare.
    mid = getattr(model, "supports_marched_event", False) and _DELAY_COPIES
    events = []
    if mid:
        for _ in range(2):
            ev = torch.cuda.Event()
            ev.record(main)   # (creates the underlying event: the library records it by handle)
            events.append(ev)

    def copy_out(o, lo):
        with torch.cuda.stream(side):
            live = [(host[j][lo:lo + t.shape[0]], t.detach().contiguous()) for j, t in enumerate(o) if t is not None and t.shape[0]]
            if _COPY_WORKGROUPS > 0 and live and all(t.dtype == torch.float32 for _h, t in live):
                # ONE small kernel writes the chunk's outputs into the pinned arrays (mapped: the device sees them through the same
                # pointer) - the runtime's copy is a kernel too, but one that fills the chip (see above)
                import ctypes as C
                from . import _lib
                n = len(live)
                src = (C.c_void_p * n)(*[t.data_ptr() for _h, t in live])
                dst = (C.c_void_p * n)(*[h.data_ptr() for h, _t in live])
                cnt = (C.c_int64 * n)(*[t.numel() for _h, t in live])
                _lib.check(_lib.load().ego_copy_out(n, src, dst, cnt, _COPY_WORKGROUPS, _lib.stream_handle()), "ego_copy_out")
            else:
                for h, t in live:
                    h.copy_(t, non_blocking=True)
            for _h, t in live:
                t.record_stream(side)   # the allocator must not hand the block out again before the copy has read it

    pending = None
    for k, lo in enumerate(range(0, max(n_all, 1), chunk)):  # an empty ray list still makes one (empty) call, so the outputs keep their shapes
        rays_chunk = rays[lo:lo + chunk].to(dev, non_blocking=True)
        extra = dict(jitter=None if jitter is None else jitter[lo:lo + chunk], u=None if u is None else u[lo:lo + chunk])
        if not keep_alpha and getattr(model, "supports_need_alpha", False):
            extra["need_alpha"] = False
        if mid:
            extra["marched_event"] = events[k & 1]
        o = model(rays_chunk, **kw, **extra)
        if not keep_alpha:
            o = o[:4] + (None,)
        if host[0] is None:
            for j, t in enumerate(o):
                if t is not None:
                    host[j] = torch.empty((n_all,) + tuple(t.shape[1:]), dtype=t.dtype, pin_memory=True)
        if mid:
            if pending is not None:   # the previous chunk is complete where this chunk's march is: its copies go under this chunk's shade
                side.wait_event(events[k & 1])
                copy_out(*pending)
            pending = (o, lo)
        else:
            side.wait_stream(main)   # chunk k's copies start when its kernels are done; chunk k + 1's kernels are queued behind them on `main`
            copy_out(o, lo)
    if pending is not None:
        side.wait_stream(main)
        copy_out(*pending)
    side.synchronize()
    main.synchronize()
    return tuple(None if h is None else h.numpy() for h in host)


# workgroups of ego_copy_out per chunk; 0: the runtime's hipMemcpyAsync.  M rays/s at 4096 x 512 with alpha copied back, one box: runtime copy
# 5.1-5.3, 128 workgroups 6.2, 32: 6.3, 16: 6.5, 8: 6.7, 4: 7.26, 3: 7.1, 2: 6.7, 1: 5.5 (resident: 7.69) - alone, four workgroups move the
# 8 MB in 172 us (49 GB/s); under the shade kernel in 540 us, just inside the chunk's 560
_COPY_WORKGROUPS = int(__import__("os").environ.get("EGO_HANDOVER_WORKGROUPS", "4"))
_DELAY_COPIES = __import__("os").environ.get("EGO_HANDOVER_DELAY", "1") != "0"   # 0: copies start as soon as their chunk is done (round 6's first form)


_COPY_STREAMS: dict = {}


def _copy_stream(dev):
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _COPY_STREAMS:
        _COPY_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return _COPY_STREAMS[idx]


def erp_rays(H: int, W: int, c2w, device, row0: int = 0, n_rows: Optional[int] = None, normalize: bool = True) -> torch.Tensor:
    """[n_rows*W, 6] rays of an equirectangular camera, generated on the device (no [H*W,6] host transfer):
    dataLoader/ray_utils.py:24-40 (get_ray_directions_360) + :85-113 (get_rays); `normalize` = the division by the norm both
    ERP datasets apply to the camera directions first (dataset_egocentric_video.py:57-58, dataset_omniblender.py:42-43)."""
    import ctypes
    from . import _lib
    n_rows = H - row0 if n_rows is None else n_rows
    pose = (ctypes.c_float * 12)(*[float(v) for v in np.asarray(c2w, dtype=np.float32).reshape(-1)[:12]])
    rays = torch.empty(n_rows * W, 6, device=device, dtype=torch.float32)
    with torch.cuda.device(rays.device):
        _lib.check(_lib.load().ego_erp_rays(H, W, row0, n_rows, pose, int(bool(normalize)), rays.data_ptr(), _lib.stream_handle()), "ego_erp_rays")
    return rays


# camera paths (renderer.py:199-255, evaluation_path): egonerf_amd/camera.py
from .camera import FrameRenderer, camera_rays, evaluation_path, finish_frame  # noqa: E402,F401


# ---------------------------------------------------------------------------------------------------
# ray sharding + PSNR reduction (one process per GPU)
# ---------------------------------------------------------------------------------------------------
def shard_bounds(n: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous, balanced block [lo, hi) of n rays for `rank` (first n % world ranks get one extra)."""
    base, extra = divmod(n, world_size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def psnr_from_sse(sse: float, count: float) -> float:
    """renderer.py:156-157: -10 log10(mean squared error)."""
    return float(-10.0 * np.log(sse / count) / np.log(10.0))


def sharded_render(render_fn: Callable[[torch.Tensor], torch.Tensor], rays: torch.Tensor, gt: Optional[torch.Tensor] = None,
                   gather_image=False, group=None):
    """Each rank renders its block of `rays` with `render_fn(rays_block) -> rgb [n,3]`.

    Returns dict(rgb_local, lo, hi, psnr (if gt given; identical on every rank), image (if gather_image: on rank 0, or on every
    rank with gather_image="all")).  No data-path collective: only the [sse, count] all-reduce and the optional tile gather.
    """
    import torch.distributed as dist

    distributed = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    lo, hi = shard_bounds(rays.shape[0], world, rank)
    rgb = render_fn(rays[lo:hi])
    if isinstance(rgb, np.ndarray):  # a render_fn built on volume_renderer(empty_gpu_cache=True)
        rgb = torch.from_numpy(rgb).to(rays.device if rays.is_cuda else "cpu")
    out = dict(rgb_local=rgb, lo=lo, hi=hi)
    if gt is not None:
        diff = rgb.double().clamp(0.0, 1.0) - gt[lo:hi].to(rgb.device).double()
        stat = torch.stack([(diff * diff).sum(), torch.tensor(float(diff.numel()), device=rgb.device, dtype=torch.float64)])
        if distributed:
            dist.all_reduce(stat, op=dist.ReduceOp.SUM, group=group)
        out["psnr"] = psnr_from_sse(stat[0].item(), stat[1].item())
    if gather_image:
        if distributed:
            sizes = [shard_bounds(rays.shape[0], world, r) for r in range(world)]
            pad = max(h - l for l, h in sizes)
            buf = torch.zeros(pad, 3, device=rgb.device, dtype=rgb.dtype)
            buf[: hi - lo] = rgb
            if gather_image == "all":   # every rank gets the image (row-sharded SSIM in evaluation())
                tiles = [torch.empty_like(buf) for _ in range(world)]
                dist.all_gather(tiles, buf, group=group)
            else:
                tiles = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
                dist.gather(buf, tiles, dst=0, group=group)
            if tiles is not None:
                out["image"] = torch.cat([t[: h - l] for t, (l, h) in zip(tiles, sizes)])
        else:
            out["image"] = rgb
    return out


@torch.no_grad()
def evaluation_psnr(images_rays: Sequence[torch.Tensor], images_gt: Sequence[torch.Tensor], model, chunk=4096, device="cuda",
                    **render_kw) -> List[float]:
    """Per-image PSNR list with renderer.py:125-157 semantics (render -> clamp -> MSE -> dB), rays sharded over
    the ranks of the default process group when one is initialised."""
    psnrs = []
    render_kw = dict(render_kw, empty_gpu_cache=False)  # the reductions below need device tensors, not the numpy D2H variant
    for rays, gt in zip(images_rays, images_gt):
        fn = lambda block: volume_renderer(block, model, chunk=chunk, device=device, keep_alpha=False, **render_kw)[0]
        psnrs.append(sharded_render(fn, rays.view(-1, rays.shape[-1]), gt.view(-1, 3))["psnr"])
    return psnrs


def sharded_image_metrics(img: torch.Tensor, ref: torch.Tensor, ws: bool, filter_size: int = 11, group=None):
    """SSIM (utils.py:106-152) and, with `ws`, WS-PSNR / WS-SSIM (extra/ws_ssim.py weights) of two [H, W, 3] images that EVERY rank
    holds, with the work split by rows: rank r evaluates rows [lo, hi) of the 'valid' SSIM map from image rows [lo, hi + fs - 1)
    and its share of the weighted squared error; three small float64 all-reduces combine them, so every rank returns the same
    (ssim, ws_psnr | None, ws_ssim | None).  Without a process group it is the plain single-process computation."""
    import torch.distributed as dist
    from .metrics import rgb_ssim, ws_weights
    distributed = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    H, W = img.shape[:2]
    Ho, Wo = H - filter_size + 1, W - filter_size + 1
    lo, hi = shard_bounds(Ho, world, rank)
    stat = torch.zeros(5, dtype=torch.float64, device=img.device)  # sum ssim | sum w * ssim, sum w (map) | sum w * d^2, sum w (pixels)
    if hi > lo:
        a, b = img[lo:hi + filter_size - 1], ref[lo:hi + filter_size - 1]
        if not ws:   # the kernel's own float64 sum of the map (no float32 map round trip)
            stat[0] = rgb_ssim(a, b, 1, filter_size) * ((hi - lo) * Wo * 3)
        else:
            smap = rgb_ssim(a, b, 1, filter_size, return_map=True).to(torch.float64)
            stat[0] = smap.sum()
            w = torch.as_tensor(ws_weights(hi - lo, filter_size // 2 + lo, H), dtype=torch.float64, device=img.device)
            stat[1] = (smap.mean(-1) * w[:, None]).sum()
            stat[2] = w.sum() * Wo
    if ws:
        plo, phi = shard_bounds(H, world, rank)
        if phi > plo:
            w = torch.as_tensor(ws_weights(phi - plo, plo, H), dtype=torch.float64, device=img.device)
            d = img[plo:phi].to(torch.float64) - ref[plo:phi].to(torch.float64)
            stat[3] = ((d * d).sum((1, 2)) * w).sum()
            stat[4] = w.sum() * W * 3
    if distributed:
        dist.all_reduce(stat, op=dist.ReduceOp.SUM, group=group)
    ssim = float(stat[0].item() / (Ho * Wo * 3))
    if not ws:
        return ssim, None, None
    return ssim, float(10.0 * np.log10(1.0 / (stat[3].item() / stat[4].item()))), float(stat[1].item() / stat[2].item())


@torch.no_grad()
def evaluation(images_rays: Sequence[torch.Tensor], images_gt: Sequence[torch.Tensor], img_wh: Tuple[int, int], model, chunk=4096,
               device="cuda", compute_extra_metrics=True, ws_metrics=False, **render_kw):
    """renderer.py:82-196 without the file output: per image render -> clamp -> PSNR (:156-157) and, with
    compute_extra_metrics, rgb_ssim (:160; LPIPS omitted).  Rays are sharded over the ranks of the default process group; for the
    windowed metrics the tiles are all-gathered (25 MB per 1024 x 2048 image) and every rank evaluates its block of rows of the
    SSIM map (sharded_image_metrics), so no rank idles while rank 0 filters a whole image.  Returns (PSNRs, ssims); with
    ws_metrics=True (the reference's `TODO: add WS-PSNR, WS-SSIM`, renderer.py:89, with extra/ws_ssim.py's latitude weights)
    (PSNRs, ssims, ws_psnrs, ws_ssims) for equirectangular images.  Every rank returns the same lists."""
    W, H = img_wh
    was_training = model.training
    model.eval()
    psnrs, ssims, wpsnrs, wssims = [], [], [], []
    render_kw = dict(render_kw, empty_gpu_cache=False)  # see evaluation_psnr
    for rays, gt in zip(images_rays, images_gt):
        fn = lambda block: volume_renderer(block, model, chunk=chunk, device=device, keep_alpha=False, **render_kw)[0]
        extra = compute_extra_metrics or ws_metrics
        out = sharded_render(fn, rays.view(-1, rays.shape[-1]), gt.view(-1, 3), gather_image="all" if extra else False)
        psnrs.append(out["psnr"])
        if extra:
            img = out["image"].clamp(0.0, 1.0).reshape(H, W, 3)
            ssim, wp, wsim = sharded_image_metrics(img, gt.view(H, W, 3).to(img.device), ws_metrics)
            if compute_extra_metrics:
                ssims.append(ssim)
            if ws_metrics:
                wpsnrs.append(wp)
                wssims.append(wsim)
    model.train(was_training)
    return (psnrs, ssims, wpsnrs, wssims) if ws_metrics else (psnrs, ssims)
