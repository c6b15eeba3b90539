"""Training step of the render path: forward with kept activations + backward (the autograd of
EgoNeRF.forward that train.py:312-314 runs in the reference).

The differentiable call is a `torch.autograd.Function` whose forward is the same kernel sequence as inference
(coarse march on the pooled tables -> inverse-CDF resampling -> fine march -> shade -> composite; the fine
sample positions are detached like EgoNeRF.py:534) plus one sort of the step's samples by texel cell on a side stream
(DESIGN.md 4.2).  Its backward runs `ego_march_backward` (compositing + density), `ego_shade_backward` (MLP / basis data
gradients on the fp16-split MFMA path) and, on the side stream, the two table scatters: sorted, atomic-free and
bit-reproducible by default (`ego_scatter_*_sorted`; the appearance walk also produces d(basis) and re-derives dv), float
atomics for `model.deterministic_scatter = False` and table shapes the sorted kernels are not built for.  The MLP weight and
bias gradients come from `ego_weight_grad` (csrc/ego_wgrad.hip), un-permuted with the column maps of `ego_train_layout`.
`forward` records every decision that shapes the step in one `StepPlan`; `backward` only reads it.
Rays that require grad receive d loss / d (origin, direction) from `ego_view_grad` + `ego_ray_grad`; when they alone ask for a
gradient (a frozen model being localised) the step has no sort, no scatter and no weight-gradient pass.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import warnings
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .field_tables import tables as table_params  # (tests and tools import table_params from here too)
from ._lib import SideStream, grad_struct as _grad_struct  # noqa: F401  (tests and tools import _grad_struct from here)


@functools.lru_cache(maxsize=None)
def _layout(which: int, n: int, device) -> torch.Tensor:
    buf = (C.c_int32 * n)()
    _lib.check(_lib.load().ego_train_layout(which, buf, n), "ego_train_layout")
    return torch.from_numpy(np.frombuffer(buf, dtype=np.int32).astype(np.int64).copy()).to(device)


_INDEX_CACHE = {}


def _env_on(name: str, default: str) -> bool:
    return os.environ.get(name, default) != "0"


# The module switches: attributes read when a step is planned (callers and tests set them at run time); the environment gives the defaults.
# The table scatters (and the forward's sort) run on a side stream next to the shade backward and the weight-gradient passes (`_lib.SideStream`)
SIDE_STREAM_SCATTER = _env_on("EGO_TRAIN_SIDE_STREAM", "1")
# d(basis) rides along in the sorted appearance walk (v is in its registers): no v dump, no d(basis) weight-gradient pass; off = dump + ego_weight_grad
WALK_BASIS = _env_on("EGO_TRAIN_WALK_BASIS", "1")
# ... and the walk re-derives dv = basis^T dfe too, so ego_shade_backward writes no dv (576 B per sample); off = the dv hand-over
WALK_DV = _env_on("EGO_TRAIN_WALK_DV", "1")
# keep the forward's x dump (rounds 1-4) instead of re-deriving x for d(W1) from the feature slots and the view direction (ego_weight_grad_x)
DUMP_X = _env_on("EGO_TRAIN_DUMP_X", "0")
# debugging: synchronise and print after every library call
_DEBUG_SYNC = _env_on("EGO_TRAIN_DEBUG_SYNC", "0")

# Optional per-call timing (bench.py): when KERNEL_MARKS is a list, an event is recorded on the current stream after every library
# call of the step and appended as (name, event); the interval between two consecutive marks is that call's kernel time plus the
# torch glue (zero fills, index scatters) queued in front of it.  Meaningful with SIDE_STREAM_SCATTER = False (one stream).
KERNEL_MARKS = None


def mark(what: str) -> None:
    """An extra mark (e.g. "begin") for callers that collect KERNEL_MARKS."""
    if KERNEL_MARKS is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        KERNEL_MARKS.append((what, ev))


def _chk(code: int, what: str) -> None:
    _lib.check(code, what)
    if _DEBUG_SYNC and not torch.cuda.is_current_stream_capturing():
        print("[ego train] queued", what, flush=True)
        torch.cuda.synchronize()
        print("[ego train] done  ", what, flush=True)
    mark(what)


# Weight-gradient products of one step land in ONE zero-filled buffer [352][160] (rows: do^T h2 | dh2^T h1 | dh1^T x | dfe^T v) and
# ONE gather turns it into the eight reference-shaped gradients (basis yin / yang, w1, b1, w2, b2, w3, b3): two small kernels
# instead of a zero fill per product and a fill + an index_put per gradient (22 launches of ~5 us each on the critical path).
_G_ROWS = dict(G3=(0, 32), G2=(32, 160), G1=(160, 288), Gb=(288, 352))
_G_LD = 160


def _gather_plan(model, device, basis_reference_columns: bool = False):
    """(flat gather index, split sizes, shapes, pad column) derived once from the layouts (no host synchronisation per step).
    basis_reference_columns: the Gb block's columns are already plane x 48 + channel (ego_scatter_app_sorted's gbasis) instead of the
    v dump's column order (ego_weight_grad over ego_shade_dump.v)."""
    key = (str(device), bool(basis_reference_columns))
    if key not in _INDEX_CACHE:
        hid, xmap, fmap, vmap = (_layout(w, n, "cpu") for w, n in ((1, 128), (0, 160), (2, 32), (3, 144)))
        x_sel = (xmap >= 0).nonzero().flatten()
        f_sel = (fmap >= 0).nonzero().flatten()
        x_cols, f_rows, pad = xmap[x_sel], fmap[f_sel], int((xmap < 0).nonzero()[0])
        src = torch.arange(352 * _G_LD).view(352, _G_LD)   # every element of the product buffer, by flat position
        G3, G2, G1, Gb = (src[a:b] for a, b in (_G_ROWS[k] for k in ("G3", "G2", "G1", "Gb")))
        mlp = model.renderModule.mlp
        neg = lambda *shape: torch.full(shape, -1, dtype=torch.int64)
        gw3 = neg(*mlp[4].weight.shape); gw3[:, hid] = G3[:3, :128]
        gb3 = G3[:3, 128].clone()
        gw2 = neg(*mlp[2].weight.shape); gw2[hid[:, None], hid[None, :]] = G2[:, :128]
        gb2 = neg(*mlp[2].bias.shape); gb2[hid] = G2[:, 128]
        gw1 = neg(*mlp[0].weight.shape); gw1[hid[:, None], x_cols[None, :]] = G1[:, x_sel]
        gb1 = neg(*mlp[0].bias.shape); gb1[hid] = G1[:, pad]
        gbasis = []
        for g in range(2):
            gb = neg(model.app_dim, 144)
            cols = torch.arange(144) if basis_reference_columns else vmap
            gb[f_rows[:, None], cols[None, :]] = Gb[32 * g: 32 * g + 32, :144][f_sel]
            gbasis.append(gb)
        parts = gbasis + [gw1, gb1, gw2, gb2, gw3, gb3]
        flat = torch.cat([p.reshape(-1) for p in parts])
        assert int(flat.min()) >= 0, "every weight / bias gradient element has a source in the product buffer"
        _INDEX_CACHE[key] = (flat.to(device), [p.numel() for p in parts], [tuple(p.shape) for p in parts], pad)
    return _INDEX_CACHE[key]


def _zeros_like_many(tensors, zero: bool = True):
    """One zero-filled flat buffer carved into tensors with the shapes AND strides of `tensors` (dense, e.g. channel-last
    parameters): one fill kernel instead of one per gradient.  zero=False: uninitialised (the sorted scatters write every texel)."""
    total = sum(t.numel() for t in tensors)
    flat = (torch.zeros if zero else torch.empty)(total, device=tensors[0].device, dtype=tensors[0].dtype)
    out, off = [], 0
    for t in tensors:
        out.append(torch.as_strided(flat, t.shape, t.stride(), off))
        assert out[-1].stride() == t.stride()
        off += t.numel()
    return out


def _empty(device, *shape, dtype=torch.float32) -> torch.Tensor:
    return torch.empty(*shape, device=device, dtype=dtype)


def differentiable_params(model) -> List[torch.nn.Parameter]:
    """Fixed order: 12 density tables, 12 appearance tables, basis yin/yang, mlp (w0,b0,w1,b1,w2,b2)."""
    head = [model.basis_mat_yin.weight, model.basis_mat_yang.weight]
    if model.shadingMode != "RGB":   # RGBRender has no parameters (tensorBase.py:37-39)
        m = model.renderModule.mlp
        head += [m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias]
    return table_params(model, "density") + table_params(model, "app") + head


def _generic_head_sorted_app(model, sort_ws, M: int) -> bool:
    """A head of another shape over 48-component appearance tables: ego_shade_backward_generic writes the blocked dv and the sorted walk
    scatters it (the step's sort exists whenever the density field has its tuned shape; sort_ws: its workspace, or True for "it will").
    Also what lets the tuned head's walk take dfe.  EGO_SORTED_WALK is read here and nowhere else, once per step when the step is planned
    (not at import: the library reads it per call too, csrc/ego_sorted_geom.h::walk_wanted, and the two must agree)."""
    return sort_ws is not None and _env_on("EGO_SORTED_WALK", "1") and model.app_n_comp[0] == 48 and (M + 31) // 32 * 32 * 144 < 2 ** 30


class StepPlan(NamedTuple):
    """Every decision that shapes one training step, taken once in RenderFunction.forward; the backward reads it and re-derives nothing."""
    N: int
    S: int
    M: int                   # N * S samples
    Mp: int                  # ... padded to whole 32-sample tiles (the tuned dumps are tile-blocked: include/egonerf_hip.h, ego_shade_dump)
    head_tuned: bool         # the MFMA head kernels (else the fp32 compatibility kernels: another shape, or the parity mode)
    compat: Optional[torch.Tensor]   # parity mode (model.train_fp32_head): the tuned head's weights packed in the compatibility layout
    sorts: bool              # the step's samples are binned by texel cell (ego_scatter_sort) for the deterministic scatters
    sorted_dens: bool        # density / appearance table gradients by the sorted, atomic-free scatter (else float atomics into zeros)
    sorted_app: bool
    walk_basis: bool         # the appearance walk produces d(basis): no v dump, no d(basis) weight-gradient pass
    walk_dv: bool            # ... and re-derives dv from dfe: ego_shade_backward writes no dv
    dump_x: bool             # the forward dumps x / v for the weight gradients
    dump_v: bool
    side: Optional["torch.cuda.Stream"]   # where the sort and the scatters run (None: in line)


def _plan_step(model, sc, N: int, S: int, param_grads: bool = True) -> StepPlan:
    """param_grads = False (a frozen model being localised: only the rays ask for a gradient): no sort, the backward runs no scatter."""
    M, device = N * S, model.density_plane_yin[0].device
    head_tuned = model.head_is_tuned and not model.train_fp32_head
    dens16 = model.density_n_comp[0] == 16
    # Deterministic table gradients (model.deterministic_scatter, the default): tuned table shapes only (16 / 48 components); anything
    # else keeps the atomic scatters
    sorts = bool(param_grads and model.deterministic_scatter and (dens16 or head_tuned))
    walk = _generic_head_sorted_app(model, sorts or None, M)
    walk_basis = bool(head_tuned and WALK_BASIS and walk)
    compat = None
    if model.head_is_tuned and not head_tuned:
        compat = _empty(device, _lib.load().ego_packed_floats_compat(sc))
    return StepPlan(N=N, S=S, M=M, Mp=(M + 31) // 32 * 32, head_tuned=head_tuned, compat=compat, sorts=sorts, sorted_dens=sorts and dens16,
                    sorted_app=sorts and (head_tuned or walk), walk_basis=walk_basis, walk_dv=bool(walk_basis and WALK_DV),
                    dump_x=bool(DUMP_X) if head_tuned else model.shadingMode != "RGB", dump_v=not walk_basis,
                    side=_lib.side_stream(device) if SIDE_STREAM_SCATTER else None)


def _head_scene(sc, plan: StepPlan, pack: bool = False) -> "_lib.Scene":
    """The scene the head's kernels see.  Parity mode (model.train_fp32_head / EGO_TRAIN_FP32=1): the tuned head trained through the fp32 compatibility
    kernels - fp32 activations, fp32 dumps, fp32 weight-gradient operands like the reference's autograd - on a copy of the
    scene whose packed blob is the compatibility layout (the tuned path keeps x / h1 / h2 / dh1 / dh2 as halves: DESIGN.md 4.2)."""
    if plan.compat is not None:
        sc = _lib.Scene.from_buffer_copy(sc)
        if pack:
            _chk(_lib.load().ego_pack_mlp_compat(sc, plan.compat.data_ptr(), _lib.stream_handle()), "ego_pack_mlp_compat")
        sc.packed = plan.compat.data_ptr()
    return sc


def _warn_inference_precision(model) -> None:
    """mlp_precision is an INFERENCE switch; before r05 a differentiable call with "f32" raised, now it would silently
    train through split-fp16 products and half-precision activation dumps - say so once, and say what the real switch is."""
    if model._mlp_precision == "f32" and not model.train_fp32_head and not getattr(model, "_warned_f32_training", False):
        warnings.warn("EgoNeRF.mlp_precision = 'f32' applies to inference only: the differentiable path runs the f16x3 training kernels "
                      "(fp16-split MFMA products, half-precision activation dumps).  For fp32 activations and operands in training set "
                      "model.train_fp32_head = True (or EGO_TRAIN_FP32=1): the parity mode, several times slower.", RuntimeWarning, stacklevel=4)
        model._warned_f32_training = True


# One operand of an A^T B weight-gradient product (ego_weight_grad_det): pointer, leading dimension, columns used, layout code
# (include/egonerf_hip.h: 0 row-major fp32, 1 / 2 the tuned dumps' fp32 / half order, 3 dfe routed by coords.w), per-sample scale
_Operand = collections.namedtuple("_Operand", "ptr ld cols layout scale", defaults=(0, None))


def _weight_grad(G, A, B, ones_col: int, M: int, part) -> None:
    """G [rows][_G_LD] += A^T [B | 1 at ones_col].  part: the workgroups' partial products, added in a fixed order (deterministic mode,
    model.deterministic_scatter) instead of float atomics."""
    _chk(_lib.load().ego_weight_grad_det(A.ptr, A.ld, A.cols, A.layout, A.scale, B.ptr, B.ld, B.cols, B.layout, ones_col, M, G.data_ptr(), _G_LD,
                                         _lib.ptr(part), 0 if part is None else part.numel(), _lib.stream_handle()), "ego_weight_grad")


def _march(plan: StepPlan, sc, model, rays, opts) -> dict:
    """coarse march on the pooled tables -> pdf merge -> fine march, or one march: z, alpha, weight, sigma, bg, coords of the step's samples."""
    lib, st, dev, N, S = _lib.load(), _lib.stream_handle(), rays.device, plan.N, plan.S
    n_coarse, zc_in = opts["n_coarse"], opts.get("z_coarse")  # explicit first-pass distances (exp_sampling=False) instead of schedule + jitter
    near = float(model.near_far[0])
    sched, jitter = (model._sched(n_coarse, dev).data_ptr(), _lib.ptr(opts["jitter"])) if zc_in is None else (None, None)
    b = dict(z=_empty(dev, N, S), alpha=_empty(dev, N, S + int(model.envmap is not None)), weight=_empty(dev, N, S), sigma=_empty(dev, N, S),
             bg=_empty(dev, N), coords=_empty(dev, N, S, 4))
    outs = (b["alpha"].data_ptr(), b["alpha"].shape[1], b["weight"].data_ptr(), b["bg"].data_ptr(), b["coords"].data_ptr(), b["sigma"].data_ptr())
    if opts["resampling"]:
        zc, wc = (_empty(dev, N, n_coarse) if zc_in is None else zc_in), _empty(dev, N, n_coarse)
        _chk(lib.ego_march_density(sc, rays.data_ptr(), N, n_coarse, _lib.ptr(zc_in), sched, jitter, near, 1, zc.data_ptr() if zc_in is None else None,
                                   None, 0, wc.data_ptr(), None, None, None, None, st), "ego_march_density")
        _chk(lib.ego_sample_pdf_merge(zc.data_ptr(), wc.data_ptr(), _lib.ptr(opts["u"]), N, n_coarse, opts["n_fine"], int(opts["use_coarse_sample"]),
                                      b["z"].data_ptr(), None, st), "ego_sample_pdf_merge")
        # fine pass: full tables and the full-resolution r grid (bit 1; EgoNeRF.py:546 normalises without `downsample`)
        _chk(lib.ego_march_density(sc, rays.data_ptr(), N, S, b["z"].data_ptr(), None, None, near, 2, None, *outs, None, st), "ego_march_density")
    else:
        _chk(lib.ego_march_density(sc, rays.data_ptr(), N, S, _lib.ptr(zc_in), sched, jitter, near, 0, b["z"].data_ptr(), *outs, None, st),
             "ego_march_density")
    return b


def _sort(plan: StepPlan, sc, coords) -> Optional[torch.Tensor]:
    """The step's samples binned by texel cell once, from the coordinates the march just wrote - on the side stream, next to the dumping
    shade forward - so that the backward's two scatters write every gradient texel once, in a fixed order (csrc/ego_scatter_sort.hip)."""
    if not plan.sorts:
        return None
    lib, N, S = _lib.load(), plan.N, plan.S
    nbytes = lib.ego_scatter_sorted_workspace_bytes(sc, N, S)
    if nbytes <= 0:
        raise RuntimeError("ego_scatter_sorted_workspace_bytes rejected the scene: " + lib.ego_last_error().decode())
    ws = _empty(coords.device, nbytes, dtype=torch.uint8)
    side = SideStream(plan.side, coords.device)
    side.run(lambda s: _chk(lib.ego_scatter_sort(sc, coords.data_ptr(), N, S, ws.data_ptr(), nbytes, s), "ego_scatter_sort"))
    side.leave_in_flight(ws, coords)   # no join here (the backward's scatters queue behind the sort): a forward whose backward never runs
    return ws


def _shade_tuned(plan: StepPlan, sc, rays, b, rgb) -> dict:
    """The MFMA shade with its tile-blocked dumps: h1 / h2 (x only with DUMP_X: d(W1) re-derives it from the feature slots `fe` and the view
    direction, ego_weight_grad_x: bit-identical operands, 0.67 GB less written and 0.4 GB less read per 8192 x 256 step) as halves in the
    kernels' operand order, v unless the appearance walk produces d(basis)."""
    dev, Mp = rays.device, plan.Mp
    f16 = lambda *shape: _empty(dev, *shape, dtype=torch.float16)
    dump = dict(x=f16(Mp, 160) if plan.dump_x else None, h1=f16(Mp, 128), h2=f16(Mp, 128), v=_empty(dev, Mp, 144) if plan.dump_v else None,
                relu_bits=_empty(dev, Mp // 32, 2, 64, 2, dtype=torch.int32), fe=_empty(dev, Mp // 32, 4, 64, 4))
    _chk(_lib.load().ego_shade(sc, rays.data_ptr(), b["z"].data_ptr(), b["coords"].data_ptr(), plan.N, plan.S, rgb.data_ptr(),
                               C.byref(_shade_dump(dump)), None, _lib.stream_handle()), "ego_shade")
    return dump


def _shade_dump(sv: dict) -> "_lib.ShadeDump":
    return _lib.ShadeDump(*(_lib.ptr(sv[k]) for k in ("x", "h1", "h2", "v", "relu_bits", "fe")))


def _shade_generic(plan: StepPlan, sc, model, rays, b, rgb) -> dict:
    """Any other model shape (opt.py:87-100): fp32 compatibility kernels over row-major dumps, padded to whole 160-column blocks (what
    ego_weight_grad multiplies at a time) with at least one zero column left for the bias gradients."""
    ldx = (model.head_in_mlpC // _G_LD + 1) * _G_LD
    z0 = lambda *shape: torch.zeros(*shape, device=rays.device, dtype=torch.float32)
    # shadingMode "RGB", no network (not dump_x): only the plane x line products are kept (they feed the basis gradient)
    dump = dict(x=z0(plan.M, ldx), h1=z0(plan.M, _G_LD), h2=z0(plan.M, _G_LD)) if plan.dump_x else dict(x=None, h1=None, h2=None)
    dump["v"] = z0(plan.M, _G_LD)
    _chk(_lib.load().ego_shade_train_generic(sc, rays.data_ptr(), b["coords"].data_ptr(), plan.N, plan.S, rgb.data_ptr(), _lib.ptr(dump["x"]), ldx,
                                             _lib.ptr(dump["h1"]), _lib.ptr(dump["h2"]), _G_LD, dump["v"].data_ptr(), _G_LD, _lib.stream_handle()),
         "ego_shade_train_generic")
    return dump


def _scatter_tables(plan: StepPlan, sc, sv, side: SideStream, kind: str, d, g_tables, walk=(None, None, None, 0)) -> None:
    """The table gradients of one field ("density": d = dfeat, "app": d = dv or None) on the side stream: the sorted scatter, the
    float-atomic one of the tuned shape, or the any-shape atomics.  walk (tuned head, sorted): (max |dv|, dfe, d(basis) block, its ld)."""
    lib, N, S, coords, ws, g = _lib.load(), plan.N, plan.S, sv["coords"].data_ptr(), sv["sort_ws"], _grad_struct(g_tables)
    density = kind == "density"
    if density and plan.sorted_dens:
        what = "ego_scatter_density_sorted"
        call = lambda s: lib.ego_scatter_density_sorted(sc, C.byref(g), coords, d.data_ptr(), N, S, ws.data_ptr(), ws.numel(), s)
    elif density and sc.density.n_comp == 16:
        what, call = "ego_scatter_density", lambda s: lib.ego_scatter_density(sc, C.byref(g), coords, d.data_ptr(), N, S, s)
    elif not density and plan.sorted_app:
        what = "ego_scatter_app_sorted" if plan.head_tuned else "ego_scatter_app_sorted(generic head)"
        call = lambda s: lib.ego_scatter_app_sorted(sc, C.byref(g), coords, _lib.ptr(d), *walk, N, S, ws.data_ptr(), ws.numel(), s)
    elif not density and plan.head_tuned:
        what, call = "ego_scatter_app", lambda s: lib.ego_scatter_app(sc, C.byref(g), coords, d.data_ptr(), N, S, s)
    else:
        field, ld = (sc.density, 0) if density else (sc.app, _G_LD)
        what, call = f"ego_scatter_generic({kind})", lambda s: lib.ego_scatter_generic(C.byref(field), C.byref(g), coords, d.data_ptr(), ld, N, S, s)
    side.run(lambda s: _chk(call(s), what))


def _head_backward_tuned(plan: StepPlan, sc, sv, dc, g_app, side: SideStream, scatter: bool = True) -> dict:
    """ego_shade_backward, then the appearance scatter on the side stream -> what the weight gradients read.  dh2 / dh1: scaled fp16 in
    the kernel's own operand order + one power of two per sample (include/egonerf_hip.h); dv: blocked fp32, not written with walk_dv.
    scatter = False (no parameter asks for a gradient): the data gradients only - no dv, no product buffer, no scatter."""
    lib, st, dev, M, Mp = _lib.load(), _lib.stream_handle(), dc.device, plan.M, plan.Mp
    tp = _empty(dev, lib.ego_train_packed_floats())
    _chk(lib.ego_pack_train(sc, tp.data_ptr(), st), "ego_pack_train")
    f16 = lambda *shape: _empty(dev, *shape, dtype=torch.float16)
    hb = dict(dh2=f16(Mp, 128), dh1=f16(Mp, 128), dh_scale=_empty(dev, 2, Mp), dfe=_empty(dev, M, 32))
    dv = None if plan.walk_dv or not scatter else _empty(dev, Mp, 144)
    # max |dv| (walk_dv: max |dfe|), found by the backward while it holds the values: the sorted scatter's fixed-point unit comes from it
    hb["dv_absmax"] = _empty(dev, 1)
    _chk(lib.ego_shade_backward(sc, tp.data_ptr(), sv["coords"].data_ptr(), dc.data_ptr(), sv["rgb"].data_ptr(), C.byref(_shade_dump(sv)),
                                hb["dh2"].data_ptr(), hb["dh1"].data_ptr(), hb["dh_scale"].data_ptr(), hb["dfe"].data_ptr(), _lib.ptr(dv),
                                hb["dv_absmax"].data_ptr(), plan.N, plan.S, st), "ego_shade_backward")
    if not scatter:
        return hb
    # the product buffer exists (zero-filled, on the main stream) BEFORE the side stream is allowed to write its d(basis) block into it
    hb["Gall"] = torch.zeros(352, _G_LD, device=dev)
    walk = (hb["dv_absmax"].data_ptr(), None, None, 0)
    if plan.walk_basis:
        walk = (hb["dv_absmax"].data_ptr(), hb["dfe"].data_ptr(), hb["Gall"][_G_ROWS["Gb"][0]:].data_ptr(), _G_LD)
    _scatter_tables(plan, sc, sv, side, "app", dv, g_app, walk)
    if side.side is not None:   # in line the scatter is queued and dv's block may be reused at once; the side stream reads it until the join
        hb["dv"] = dv
    return hb


def _weight_grads_tuned(plan: StepPlan, model, sv, hb, dc, side: SideStream) -> list:
    """One pass of ego_weight_grad (bf16 hi/lo MFMA over transposed LDS tiles, bias gradients from a ones column) per layer over the dumped
    buffers into one product buffer, then one gather un-permutes the lane-order columns into the reference-shaped gradients
    (basis yin, basis yang, w1, b1, w2, b2, w3, b3: differentiable_params order)."""
    M, S, Gall = plan.M, plan.S, hb["Gall"]
    G = {k: Gall[a:b] for k, (a, b) in _G_ROWS.items()}
    gidx, gsizes, gshapes, pad = _gather_plan(model, dc.device, plan.walk_basis)  # pad: a zero padding column of x doubles as the ones column
    part = _empty(dc.device, _lib.load().ego_weight_grad_partial_floats()) if model.deterministic_scatter else None
    half = lambda t, cols, scale=None: _Operand(t.data_ptr(), t.shape[1], cols, 2, _lib.ptr(scale))
    _weight_grad(G["G3"], _Operand(dc.data_ptr(), 3, 3), half(sv["h2"], 128), 128, M, part)   # dc: now d(pre-sigmoid)
    _weight_grad(G["G2"], half(hb["dh2"], 128, hb["dh_scale"][0]), half(sv["h1"], 128), 128, M, part)
    if plan.dump_x:
        _weight_grad(G["G1"], half(hb["dh1"], 128, hb["dh_scale"][1]), half(sv["x"], 160), pad, M, part)
    else:   # the layer-1 input re-derived from the feature slots and the rays' directions inside the product's B-tile fetch
        _chk(_lib.load().ego_weight_grad_x(hb["dh1"].data_ptr(), hb["dh_scale"][1].data_ptr(), sv["fe"].data_ptr(), sv["rays"].data_ptr(), S, pad, M,
                                           G["G1"].data_ptr(), _G_LD, _lib.ptr(part), 0 if part is None else part.numel(), _lib.stream_handle()),
             "ego_weight_grad")
    if plan.walk_basis:
        side.join()   # the walk's k_basis_reduce wrote Gall's Gb block on the side stream
    else:   # 32 stored columns of dfe, routed to the yin / yang block by coords.w
        _weight_grad(G["Gb"], _Operand(hb["dfe"].data_ptr(), 32, 64, 3, sv["coords"].data_ptr()), _Operand(sv["v"].data_ptr(), 144, 144, 1), -1, M, part)
    return [t.view(shp) for t, shp in zip(Gall.view(-1).index_select(0, gidx).split(gsizes), gshapes)]


def _head_backward_generic(plan: StepPlan, sc, model, sv, dc, g_app, side: SideStream, scatter: bool = True) -> dict:
    """Backward of the appearance head for any model shape the compatibility kernels support (row-major buffers).  Another head over the
    SHIPPED table shape: dv in the tuned scatters' blocked layout, and the sorted walk takes the table gradients (deterministic, 0.75 ms
    where the any-shape atomic scatter takes 9.8)."""
    dev, M, hid, rgb_head = dc.device, plan.M, model.head_hidden, not plan.dump_x
    hb = dict(dh2=None if rgb_head else _empty(dev, M, hid), dh1=None if rgb_head else _empty(dev, M, hid), dfe=_empty(dev, M, 64),
              ldx=_G_LD if rgb_head else sv["x"].shape[1])
    hb["dv"] = _empty(dev, plan.Mp, 144) if plan.sorted_app else _empty(dev, M, _G_LD)
    _chk(_lib.load().ego_shade_backward_generic(sc, sv["coords"].data_ptr(), dc.data_ptr(), sv["rgb"].data_ptr(), _lib.ptr(sv["x"]), hb["ldx"],
                                                _lib.ptr(sv["h1"]), _lib.ptr(sv["h2"]), _G_LD, _lib.ptr(hb["dh2"]), _lib.ptr(hb["dh1"]),
                                                hb["dfe"].data_ptr(), hb["dv"].data_ptr(), 0 if plan.sorted_app else _G_LD, plan.N, plan.S,
                                                _lib.stream_handle()), "ego_shade_backward_generic")
    if scatter:
        _scatter_tables(plan, sc, sv, side, "app", hb["dv"], g_app)
    return hb


def _weight_grads_generic(plan: StepPlan, model, sv, hb, dc) -> list:
    """The weight gradients as A^T B products in 160-column blocks, already in the reference's [out][in] orientation."""
    M, hid, in_c, ncol, D, ldx = plan.M, model.head_hidden, model.head_in_mlpC, 3 * model.app_n_comp[0], model.app_dim, hb["ldx"]
    hp = (hid + 31) // 32 * 32
    part = _empty(dc.device, _lib.load().ego_weight_grad_partial_floats()) if model.deterministic_scatter else None

    def product(A, ca, B_ptr, ldb, ones_col, rows):
        G = torch.zeros(rows, _G_LD, device=dc.device)
        _weight_grad(G, _Operand(A.data_ptr(), ca, ca), _Operand(B_ptr, ldb, _G_LD), ones_col, M, part)
        return G

    Gb = product(hb["dfe"], 64, sv["v"].data_ptr(), _G_LD, -1, 64)                      # [yin | yang] feature gradients ^T v
    wg = [Gb[0:D, :ncol].contiguous(), Gb[32:32 + D, :ncol].contiguous()]
    if plan.dump_x:
        G3 = product(dc.view(M, 3), 3, sv["h2"].data_ptr(), _G_LD, hid, 32)               # do^T [h2 | 1]
        G2 = product(hb["dh2"], hid, sv["h1"].data_ptr(), _G_LD, hid, hp)                 # dh2^T [h1 | 1]
        G1 = []
        for c0 in range(0, ldx, _G_LD):
            ones = in_c - c0 if c0 <= in_c < c0 + _G_LD else -1                           # the first zero-padding column doubles as the ones column
            G1.append(product(hb["dh1"], hid, sv["x"].data_ptr() + 4 * c0, ldx, ones, hp))
        G1 = torch.cat(G1, dim=1)
        wg += [G1[:hid, :in_c].contiguous(), G1[:hid, in_c].contiguous(), G2[:hid, :hid].contiguous(), G2[:hid, hid].contiguous(),
               G3[:3, :hid].contiguous(), G3[:3, hid].contiguous()]
    return wg


def _envmap_grad(sc, model, sv, g_rgb) -> torch.Tensor:
    g_em = torch.zeros_like(model.envmap.emission)
    _chk(_lib.load().ego_envmap_backward(sc, sv["rays"].data_ptr() + 12, 6, g_rgb.data_ptr(), sv["raw"].data_ptr(), sv["bg"].data_ptr(),
                                         sv["env"].data_ptr(), g_rgb.shape[0], g_em.data_ptr(), _lib.stream_handle()), "ego_envmap_backward")
    return g_em


def _ray_grad(plan: StepPlan, sc, model, sv, hb, dfeat, g_rgb, fine_pass: bool) -> torch.Tensor:
    """d loss / d rays [N, 6] from what the backward has in hand: dfeat (ego_march_backward), the head's dfe and dh1, the
    forward's coords and z.  Two launches (one for the RGB head, which has no view term), no atomics: bit-reproducible."""
    lib, st, dev, rays = _lib.load(), _lib.stream_handle(), dfeat.device, sv["rays"]
    d_view = None
    if model.shadingMode != "RGB":
        d_view = _empty(dev, plan.M, 3)
        layout, scale = (2, hb["dh_scale"][1].data_ptr()) if plan.head_tuned else (0, None)
        _chk(lib.ego_view_grad(sc, rays.data_ptr(), plan.S, plan.M, hb["dh1"].data_ptr(), layout, scale, d_view.data_ptr(), st), "ego_view_grad")
    env = (g_rgb, sv["raw"], sv["bg"], sv["env"]) if sv["env"] is not None else (None,) * 4
    g_rays = _empty(dev, plan.N, 6)
    _chk(lib.ego_ray_grad(sc, rays.data_ptr(), sv["z"].data_ptr(), sv["coords"].data_ptr(), dfeat.data_ptr(), hb["dfe"].data_ptr(),
                          hb["dfe"].shape[1], _lib.ptr(d_view), *(_lib.ptr(t) for t in env), plan.N, plan.S, int(fine_pass), None,
                          g_rays.data_ptr(), st), "ego_ray_grad")
    return g_rays


class RenderFunction(torch.autograd.Function):
    @staticmethod
    @_lib.device_guard
    def forward(ctx, model, rays, opts, *params):
        """params = differentiable_params(model) (+ envmap.emission last when the model has an envmap)."""
        lib, st, dev = _lib.load(), _lib.stream_handle(), rays.device
        ctx.set_materialize_grads(False)
        # training gathers from the fp32 parameters (the backward re-gathers from them), shades every sample like EgoNeRF.forward (the
        # appearance skip is an inference option) and keeps all three fp16 terms of every product, whatever model.mlp_precision says
        _warn_inference_precision(model)
        sc = model.scene(training=True)
        N = rays.shape[0]
        S = _lib.sample_count(opts["n_coarse"], opts["n_fine"], opts["resampling"], opts["use_coarse_sample"])
        # (needs_input_grad: model, rays, opts, *params) a frozen model whose rays ask for a gradient plans a step without the sort
        plan = _plan_step(model, sc, N, S, param_grads=any(ctx.needs_input_grad[3:]) or not ctx.needs_input_grad[1])
        b = _march(plan, sc, model, rays, opts)
        model.last_train_z = b["z"]   # the 5-tuple has no place for it; losses.distortion_loss reads it right after the render
        rgb = _empty(dev, N, S, 3)
        sort_ws = _sort(plan, sc, b["coords"])
        sc = _head_scene(sc, plan, pack=True)
        dump = _shade_tuned(plan, sc, rays, b, rgb) if plan.head_tuned else _shade_generic(plan, sc, model, rays, b, rgb)
        rgb_map, depth, raw = _empty(dev, N, 3), _empty(dev, N), _empty(dev, N, 3)
        has_env = model.envmap is not None
        bg_map, env_map = (_empty(dev, N, 3), _empty(dev, N, 3)) if has_env else (None, None)
        _chk(lib.ego_composite(sc, rays.data_ptr(), b["z"].data_ptr(), b["weight"].data_ptr(), b["bg"].data_ptr(), rgb.data_ptr(), N, S,
                               rgb_map.data_ptr(), depth.data_ptr(), _lib.ptr(bg_map), _lib.ptr(env_map), raw.data_ptr(), st), "ego_composite")
        ctx.model, ctx.plan, ctx.fine_pass = model, plan, bool(opts["resampling"])
        ctx.saved = dict(b, rgb=rgb, raw=raw, env=env_map, rays=rays, sort_ws=sort_ws, **dump)
        # depth is computed under no_grad in the reference (EgoNeRF.py:595-598); one call: a second would replace the first
        if has_env:
            ctx.mark_non_differentiable(depth, bg_map, env_map)
            return rgb_map, depth, b["alpha"], bg_map, env_map
        ctx.mark_non_differentiable(depth)
        return rgb_map, depth, b["alpha"]

    @staticmethod
    @_lib.device_guard
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, _g_depth=None, g_alpha=None, *_unused):
        model, plan, sv = ctx.model, ctx.plan, ctx.saved
        dev = sv["z"].device
        # rays: d loss / d (origin, direction) only when asked for; params: False for a frozen model being localised, whose backward is
        # ego_march_backward, the head's data-gradient kernel and the ray-gradient kernels - no scatter, no weight-gradient pass
        want_rays, want_params = ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:]) or not ctx.needs_input_grad[1]
        sc = _head_scene(model.scene(training=True), plan)
        g_rgb = torch.zeros(plan.N, 3, device=dev) if g_rgb is None else g_rgb.contiguous().float()
        if g_alpha is not None:  # ray_entropy_loss (train.py:306-309); the envmap's ones column takes no gradient
            g_alpha = g_alpha.contiguous().float()
            assert g_alpha.shape == sv["alpha"].shape
        dc, dfeat = _empty(dev, plan.N, plan.S, 3), _empty(dev, plan.N, plan.S)   # d colour (-> d(pre-sigmoid) in the head backward), d density feature
        _chk(_lib.load().ego_march_backward(sc, sv["z"].data_ptr(), sv["alpha"].data_ptr(), sv["alpha"].shape[1], sv["weight"].data_ptr(),
                                            sv["sigma"].data_ptr(), sv["bg"].data_ptr(), sv["rgb"].data_ptr(), g_rgb.data_ptr(), _lib.ptr(g_alpha),
                                            sv["raw"].data_ptr(), _lib.ptr(sv["env"]), plan.N, plan.S, dc.data_ptr(), dfeat.data_ptr(),
                                            _lib.stream_handle()), "ego_march_backward")
        side = SideStream(plan.side, dev)
        try:
            if not want_params:
                head = _head_backward_tuned if plan.head_tuned else functools.partial(_head_backward_generic, model=model)
                hb = head(plan, sc, sv=sv, dc=dc, g_app=None, side=side, scatter=False)
                return (None, _ray_grad(plan, sc, model, sv, hb, dfeat, g_rgb, ctx.fine_pass), None, *([None] * (len(ctx.needs_input_grad) - 3)))
            # keeps the channel-last strides of the parameters; the sorted scatters store every texel, the atomic ones add into zeros
            g_dens = _zeros_like_many(table_params(model, "density"), zero=not plan.sorted_dens)
            g_app = _zeros_like_many(table_params(model, "app"), zero=not plan.sorted_app)
            _scatter_tables(plan, sc, sv, side, "density", dfeat, g_dens)
            if plan.head_tuned:
                hb = _head_backward_tuned(plan, sc, sv, dc, g_app, side)
                wg = _weight_grads_tuned(plan, model, sv, hb, dc, side)
            else:
                hb = _head_backward_generic(plan, sc, model, sv, dc, g_app, side)
                wg = _weight_grads_generic(plan, model, sv, hb, dc)
            grads = g_dens + g_app + wg
            if sv["env"] is not None:
                grads.append(_envmap_grad(sc, model, sv, g_rgb))
            g_rays = _ray_grad(plan, sc, model, sv, hb, dfeat, g_rgb, ctx.fine_pass) if want_rays else None
            side.join()  # the table gradients are complete
            return (None, g_rays, None, *grads)
        finally:
            # also when a call above raised: the main stream waits for the side stream before dfeat, dv / dfe (hb), coords and sort_ws
            # (sv) and the gradient buffers can go back to the main stream's allocator pool
            side.join()
            ctx.saved = None


class EnvRadianceFunction(torch.autograd.Function):
    """EnvironmentMap.get_radiance with a gradient to `emission` (the reference's envmap pre-training, train.py:218-236)."""

    @staticmethod
    @_lib.device_guard
    def forward(ctx, emission, dirs):
        lib, st = _lib.load(), _lib.stream_handle()
        sc = _lib.new_scene()
        sc.envmap, sc.envmap_h = emission.data_ptr(), emission.shape[2]
        out = torch.empty(dirs.shape[0], 3, device=dirs.device)
        _lib.check(lib.ego_envmap_radiance(sc, dirs.data_ptr(), dirs.shape[0], out.data_ptr(), st), "ego_envmap_radiance")
        ctx.save_for_backward(dirs, out)
        ctx.shape = emission.shape
        return out

    @staticmethod
    @_lib.device_guard
    def backward(ctx, g):
        lib, st = _lib.load(), _lib.stream_handle()
        dirs, out = ctx.saved_tensors
        N = dirs.shape[0]
        sc = _lib.new_scene()
        sc.envmap_h = ctx.shape[2]
        g_em = torch.zeros(ctx.shape, device=dirs.device)
        ones, inside = torch.ones(N, device=dirs.device), torch.zeros(N, 3, device=dirs.device)
        _lib.check(lib.ego_envmap_backward(sc, dirs.data_ptr(), 3, g.contiguous().float().data_ptr(), inside.data_ptr(), ones.data_ptr(),
                                           out.data_ptr(), N, g_em.data_ptr(), st), "ego_envmap_backward")
        return g_em, None


def render_train(model, rays, n_coarse, n_fine=0, resampling=False, use_coarse_sample=True, jitter: Optional[torch.Tensor] = None,
                 u: Optional[torch.Tensor] = None, z_coarse: Optional[torch.Tensor] = None):
    """Differentiable EgoNeRF.forward (is_train semantics) -> (rgb_map, depth, bg_map|None, env_map|None, alpha).  The samples' distances
    [N, S] stay on the model as `model.last_train_z` (the march's own buffer, no gradient): losses.distortion_loss takes them."""
    opts = dict(n_coarse=int(n_coarse), n_fine=int(n_fine), resampling=bool(resampling), use_coarse_sample=bool(use_coarse_sample),
                jitter=jitter, u=u, z_coarse=z_coarse)
    params = differentiable_params(model)
    if model.envmap is not None:
        params = params + [model.envmap.emission]
    out = RenderFunction.apply(model, rays, opts, *params)
    if model.envmap is not None:
        rgb_map, depth, alpha, bg_map, env_map = out
        return rgb_map, depth, bg_map, env_map, alpha
    rgb_map, depth, alpha = out
    return rgb_map, depth, None, None, alpha


class TrainSchedule:
    """Device-side iteration clock for loss terms whose weights change from iteration to iteration.  train.py:295-309 multiplies
    TV_weight_density / TV_weight_app (while `iteration < iter_ignore_TV`) and entropy_weight (once `iteration > iter_ignore_entropy`)
    by lr_factor in every iteration in which the term is active; a Python float captured into a hipGraph would freeze at its value
    of the capture.  `it` is a float64 device scalar holding the index of the CURRENT iteration (GraphedTrainStep advances it inside
    the graph), and `decayed()` evaluates the reference's running product as a device expression."""

    def __init__(self, device, start_iteration: int = 0):
        self.first = int(start_iteration)
        self.it = torch.full((), float(start_iteration), dtype=torch.float64, device=device)

    def decayed(self, w0: float, factor: float, active_before: Optional[int] = None, active_after: Optional[int] = None) -> torch.Tensor:
        """The weight the reference's loop holds in the current iteration (float32 device scalar; 0 when the term is gated off):
        `active_before=K`: term active while iteration < K, `w *= factor` in every active iteration before use (the TV terms,
        train.py:295-304); `active_after=K`: active once iteration > K (the ray-entropy term, train.py:306-309)."""
        it = self.it
        if (active_before is None) == (active_after is None):
            raise ValueError("TrainSchedule.decayed: exactly one of active_before / active_after")
        if active_before is not None:
            n, gate = it - (self.first - 1), it < float(active_before)
        else:
            n, gate = it - float(max(int(active_after), self.first - 1)), it > float(active_after)
        w = float(w0) * torch.pow(torch.full_like(it, float(factor)), n)
        return torch.where(gate, w, torch.zeros_like(w)).float()

    def stepped(self, w0: float, rate: float, step_size: float, end_iter: Optional[int] = None) -> torch.Tensor:
        """The depth term's weight in the current iteration (float32 device scalar): `depth_lambda * depth_rate ** int(iteration /
        depth_step_size)` (train.py:276), and 0 once `iteration > depth_end_iter` (train.py:279-281, where the reference zeroes the
        term itself)."""
        it = self.it
        if not float(step_size) > 0.0:
            raise ValueError("TrainSchedule.stepped: step_size must be > 0")
        w = float(w0) * torch.pow(torch.full_like(it, float(rate)), torch.floor(it / float(step_size)))
        if end_iter is not None:
            w = torch.where(it > float(end_iter), torch.zeros_like(w), w)
        return w.float()

    def iteration(self) -> int:
        return int(self.it.item())


_GRAPHED_RAY_GRADS = ("GraphedTrainStep copies its batch into static buffers: rays that require grad get no gradient through it "
                      "(pose refinement runs the eager loop, egonerf_amd.poses.refine_poses)")


class GraphedTrainStep:
    """One training iteration of train.py:245-330 — differentiable render of a ray batch, loss, backward, optimiser step with
    the per-step learning-rate decay, coarse-table refresh — captured once as a hipGraph and replayed.

    An eager iteration queues ~150 launches (the library's kernels plus torch's fills, random numbers, loss arithmetic and
    autograd bookkeeping) from 1.3-2.0 ms of Python / ctypes time and leaves the device gaps between small kernels; a replay costs
    0.16 ms of host time and runs the same kernels 3 % faster (6.2 -> 6.03 ms per 8192-ray iteration, alternated on one box).

    The optimiser must be `FusedAdam(..., capturable=True, lr_factor=...)` (step count and lr schedule on the device).  The
    constructor runs `warmup` REAL iterations on the example batch (they train the model like any other iteration) and then
    captures one; `__call__(rays, target)` copies the batch into the graph's static inputs, replays, and returns the loss tensor
    of that iteration (overwritten by the next call).  Shapes are fixed: re-create the object after `upsample_volume_grid`
    (train.py:377-392 re-creates the optimiser there as well).  `loss_fn(rgb_map, target, alpha)` defaults to the MSE of
    train.py:250; regularisers go in there (egonerf_amd.losses).  `noise_fn` replaces torch.rand for the is_train jitter.

    Loss terms whose WEIGHTS change per iteration (train.py:295-309: the TV and ray-entropy weights decay by lr_factor per active
    iteration and are gated on iter_ignore_TV / iter_ignore_entropy) must not be Python floats - a float is frozen into the graph at
    capture.  A `loss_fn` whose fourth parameter is named `sched` / `schedule` (or any loss_fn with `schedule_aware=True`) receives `self.schedule` (a TrainSchedule: device-side iteration counter advanced
    inside the graph) and writes e.g. `sched.decayed(TV_weight_density, lr_factor, active_before=iter_ignore_TV) * model.TV_loss_density(tv)`;
    tests/test_hip_train_graph.py::test_graphed_step_with_decaying_regulariser_weights pins that against the eager loop.
    The ray-entropy term is `ray_entropy_loss(alpha) * w`.  The distortion term also needs the samples' distances, which the 5-tuple
    does not carry: every training render leaves them on the model, and the loss_fn reads them right after the render,
    `distortion_loss(alpha, model.last_train_z, model.near_far) * w` (tests/test_hip_distortion.py pins it against the eager loop).

    `batch_source` (a DeviceSimpleSampler / DeviceThetaImportanceSampler of egonerf_amd.sampler over a RayBank): the batch is drawn
    INSIDE the graph - the iteration starts with the source's one launch writing indices, rays and colours into the static buffers
    `self.idx` / `self.rays` / `self.target`, and the source's device counter is advanced next to `schedule.it` - so `rays` / `target`
    are omitted, `step()` takes no arguments and nothing crosses the host link per iteration.  `start_iteration` positions the source's
    counter as well: iteration k of a resumed run draws `batch_source.indices_at(k)`.

    Depth targets (losses.depth_loss): a `loss_fn` with a parameter NAMED `depth` receives the batch's targets as the keyword
    `depth=self.depth`, a static float32 [B] buffer.  With a `batch_source` whose bank has depths (RayBank(depths=...)) the buffer is
    filled inside the graph, by `bank.gather_depth_into(self.idx, self.depth)` right after the source's launch; with host-fed batches
    the constructor takes an example `depth=` [B] and `step(rays, target, depth=...)` copies the iteration's targets in.  A loss_fn that
    names `depth` without either source is refused at construction.  The weight of train.py:276 is `sched.stepped(depth_lambda,
    depth_rate, depth_step_size, depth_end_iter)`; the term reads `model.last_train_z` like the distortion term:
    `depth_loss(alpha, model.last_train_z, depth)` (tests/test_hip_depth_loss.py pins it against the eager loop).

    Masks and exposure (losses.photometric_loss): the same opt-in by name.  A `loss_fn` with a parameter NAMED `weight` receives
    `weight=self.weight`, a static float32 [B] buffer: with a `batch_source` whose bank has masks (RayBank(masks=...)) it is filled inside
    the graph by `bank.gather_mask_into(self.idx, self.weight)`; host-fed, the constructor takes an example `weight=` [B] and
    `step(rays, target, weight=...)` copies the iteration's in.  A parameter NAMED `image` receives `image=self.image`, a static int32
    [B] buffer: with a `batch_source` it is `bank.image_of(self.idx)` written inside the graph; host-fed it comes through `image=` in the
    same way.  Naming either without a source is refused at construction; a loss_fn that names neither runs exactly the calls it ran
    before.  The parameters of an exposure.ExposureDeltas are an ordinary extra group of the FusedAdam the step drives:
    `photometric_loss(rgb, gt, weight=weight, image=image, affine=deltas.affine())` (tests/test_hip_photo_loss.py pins it against the
    eager loop)."""

    def __init__(self, model, optimizer, rays=None, target=None, render_kwargs=None, loss_fn=None, warmup=3, noise_fn=None, start_iteration=0,
                 schedule_aware=None, batch_source=None, depth=None, weight=None, image=None):
        if not getattr(optimizer, "capturable", False):
            raise ValueError("GraphedTrainStep needs FusedAdam(capturable=True): the step count and lr schedule must live on the device")
        if render_kwargs is None:
            raise ValueError("GraphedTrainStep needs render_kwargs")
        self.source = batch_source
        if batch_source is not None:
            if rays is not None or target is not None:
                raise ValueError("GraphedTrainStep: with a batch_source the batches are drawn on the device; pass no rays / target")
            dev0 = batch_source.bank.device
            rays = torch.empty(batch_source.batch, 6, device=dev0, dtype=torch.float32)
            target = torch.empty(batch_source.batch, 3, device=dev0, dtype=torch.float32)
            self.idx = torch.empty(batch_source.batch, device=dev0, dtype=torch.int64)
            batch_source.seek(start_iteration)
            if depth is not None:
                raise ValueError("GraphedTrainStep: with a batch_source the depth targets come from its bank (RayBank(depths=...)); pass no depth")
            if getattr(batch_source.bank, "depths", None) is not None:
                depth = torch.empty(batch_source.batch, device=dev0, dtype=torch.float32)
            if weight is not None or image is not None:
                raise ValueError("GraphedTrainStep: with a batch_source the weights come from its bank (RayBank(masks=...)) and the image "
                                 "indices from its ray indices; pass no weight / image")
        elif rays is None or target is None:
            raise ValueError("GraphedTrainStep needs an example batch (rays, target) or a batch_source")
        if rays is not None and rays.requires_grad:
            raise NotImplementedError(_GRAPHED_RAY_GRADS)
        self.model, self.opt, self.kw = model, optimizer, dict(render_kwargs)
        self.loss_fn = loss_fn or (lambda rgb, tgt, alpha: torch.mean((rgb - tgt) ** 2))
        # Explicit opt-in, not arity sniffing (a fourth parameter like reduction="mean" must not receive the schedule, a
        # *args loss must be able to): `schedule_aware=True`, or - when left None - a loss_fn parameter NAMED `sched` or `schedule`.
        if schedule_aware is None:
            import inspect
            try:
                schedule_aware = any(n in ("sched", "schedule") for n in inspect.signature(self.loss_fn).parameters)
            except (TypeError, ValueError):
                schedule_aware = False
        self._loss_takes_schedule = bool(schedule_aware)
        # the same opt-in by name for the depth targets
        try:
            import inspect
            self._loss_takes_depth = "depth" in inspect.signature(self.loss_fn).parameters
        except (TypeError, ValueError):
            self._loss_takes_depth = False
        if self._loss_takes_depth and depth is None:
            raise ValueError("GraphedTrainStep: loss_fn names `depth` but there is no depth source: pass depth= with a host-fed batch, "
                             "or a batch_source whose bank has depths")
        if depth is not None and (depth.dim() != 1 or depth.shape[0] != rays.shape[0]):
            raise ValueError(f"GraphedTrainStep: depth must be [B] = [{rays.shape[0]}], got {tuple(depth.shape)}")
        self.depth = None if depth is None else depth.detach().to(rays.device).float().contiguous().clone()
        # and for the per-ray weights and image indices of the photometric term; their buffers exist only when the loss_fn asks for them
        try:
            names = inspect.signature(self.loss_fn).parameters
            self._loss_takes_weight, self._loss_takes_image = "weight" in names, "image" in names
        except (TypeError, ValueError):
            self._loss_takes_weight = self._loss_takes_image = False
        B = rays.shape[0]
        self.weight = self.image = None
        if self._loss_takes_weight:
            if batch_source is not None:
                if getattr(batch_source.bank, "masks", None) is None:
                    raise ValueError("GraphedTrainStep: loss_fn names `weight` but the batch_source's bank has no masks (RayBank(masks=...))")
                self.weight = torch.empty(B, device=rays.device, dtype=torch.float32)
            elif weight is None:
                raise ValueError("GraphedTrainStep: loss_fn names `weight` but there is no weight source: pass weight= with a host-fed "
                                 "batch, or a batch_source whose bank has masks")
            else:
                if weight.dim() != 1 or weight.shape[0] != B:
                    raise ValueError(f"GraphedTrainStep: weight must be [B] = [{B}], got {tuple(weight.shape)}")
                self.weight = weight.detach().to(rays.device).float().contiguous().clone()
        elif weight is not None:
            raise ValueError("GraphedTrainStep: weight= was given but loss_fn has no parameter named `weight`")
        if self._loss_takes_image:
            if batch_source is not None:
                self.image = torch.empty(B, device=rays.device, dtype=torch.int32)
            elif image is None:
                raise ValueError("GraphedTrainStep: loss_fn names `image` but there is no image source: pass image= with a host-fed "
                                 "batch, or a batch_source")
            else:
                if image.dim() != 1 or image.shape[0] != B or image.dtype not in (torch.int32, torch.int64):
                    raise ValueError(f"GraphedTrainStep: image must be an int32 / int64 [B] = [{B}] tensor, got {image.dtype} {tuple(image.shape)}")
                self.image = image.detach().to(rays.device, torch.int32).contiguous().clone()
        elif image is not None:
            raise ValueError("GraphedTrainStep: image= was given but loss_fn has no parameter named `image`")
        self.schedule = TrainSchedule(rays.device, start_iteration)
        # noise_fn(n_rays, n_samples, device) -> [n_rays, n_samples] in [0, 1): torch.rand by default; tests pin it
        self.noise_fn = noise_fn or (lambda n, m, dev: torch.rand(n, m, device=dev))
        self.rays, self.target = rays.detach().clone().float().contiguous(), target.detach().clone().float().contiguous()
        dev = self.rays.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):   # torch's capture recipe: warm up off the default stream
            for _ in range(max(int(warmup), 1)):
                self._iteration()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = self._iteration()
        self._params = [p for g in optimizer.param_groups for p in g["params"]]
        self.iterations = max(int(warmup), 1)  # the capture itself does not execute

    def _iteration(self):
        N = self.rays.shape[0]
        dev = self.rays.device
        kw = self.kw
        if self.source is not None:   # this iteration's batch, drawn from the source's device counter straight into the static inputs
            self.source.sample_into(self.idx, self.rays, self.target)
            if self.depth is not None:
                self.source.bank.gather_depth_into(self.idx, self.depth)
            if self.weight is not None:
                self.source.bank.gather_mask_into(self.idx, self.weight)
            if self.image is not None:
                self.image.copy_(self.source.bank.image_of(self.idx))
        # the is_train noise comes from the device generator (graph-safe: every replay draws new numbers)
        jitter = self.noise_fn(N, kw["n_coarse"], dev)
        u = self.noise_fn(N, kw["n_fine"], dev) if kw.get("resampling") else None
        rgb, _depth, _bg, _env, alpha = self.model(self.rays, is_train=True, jitter=jitter, u=u, **kw)
        extra = dict(depth=self.depth) if self._loss_takes_depth else {}
        if self._loss_takes_weight:
            extra["weight"] = self.weight
        if self._loss_takes_image:
            extra["image"] = self.image
        loss = self.loss_fn(rgb, self.target, alpha, self.schedule, **extra) if self._loss_takes_schedule else self.loss_fn(rgb, self.target, alpha, **extra)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        if kw.get("resampling"):
            self.model.update_coarse_sigma_grid()  # train.py:356-357
        self.schedule.it.add_(1.0)   # inside the graph: the next replay sees the next iteration index
        if self.source is not None:
            self.source.counter.add_(1)
        return loss.detach()

    def __call__(self, rays=None, target=None, depth=None, weight=None, image=None):
        if self.source is not None:
            if rays is not None or target is not None or depth is not None or weight is not None or image is not None:
                raise ValueError("this GraphedTrainStep draws its batches from its batch_source inside the graph: call step() without arguments")
        elif rays is None or target is None:
            raise ValueError("this GraphedTrainStep was built without a batch_source: call step(rays, target)")
        else:
            if rays.requires_grad:
                raise NotImplementedError(_GRAPHED_RAY_GRADS)
            self.rays.copy_(rays, non_blocking=True)
            self.target.copy_(target, non_blocking=True)
            if depth is not None:
                if self.depth is None:
                    raise ValueError("this GraphedTrainStep was built without depth targets: pass an example depth= to the constructor")
                self.depth.copy_(depth, non_blocking=True)
            elif self._loss_takes_depth:
                raise ValueError("this GraphedTrainStep's loss_fn takes depth targets: call step(rays, target, depth=...)")
            for name, given, buf in (("weight", weight, self.weight), ("image", image, self.image)):
                if given is not None:
                    if buf is None:
                        raise ValueError(f"this GraphedTrainStep's loss_fn takes no `{name}`: it was built without one")
                    buf.copy_(given, non_blocking=True)
                elif buf is not None:
                    raise ValueError(f"this GraphedTrainStep's loss_fn takes `{name}`: call step(rays, target, {name}=...)")
        self.graph.replay()
        self.iterations += 1
        # the replayed optimiser wrote the parameters through raw pointers: tell autograd and the model's packed-weight cache
        for p in self._params:
            torch.autograd.graph.increment_version(p)
        return self.loss
