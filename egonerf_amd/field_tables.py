"""Storage of a VM field's 12 channel-last tables: which tables make a field and in what order, how they are carved from one
buffer, and how their pointers go into the C-ABI structs.  The canonical order is that of ego_vm_field / ego_vm_grad
(include/egonerf_hip.h): plane_yin[0..2], line_yin[0..2], plane_yang[0..2], line_yang[0..2].  `list_names()` is the only place it is
written; the index `6 * grid + 3 * is_line + i` follows from it.  (The regularisers and get_optparam_groups in model.py keep the
reference's own orders: those fix floating-point sums and optimiser state.)"""
from __future__ import annotations

from typing import List

import torch


def list_names(kind: str, coarse: bool = False) -> List[str]:
    """The model attributes that hold a field's tables, three per list, in the canonical order."""
    prefix = "coarse_sigma" if coarse else kind
    return [f"{prefix}_{what}_{g}" for g in ("yin", "yang") for what in ("plane", "line")]


def tables(model, kind: str, coarse: bool = False) -> List[torch.Tensor]:
    """The 12 tensors of field `kind` ("density" | "app") in the canonical order; coarse=True: the 2x pooled `coarse_sigma_*`
    tables of the density field (None entries before the first update_coarse_sigma_grid())."""
    return [t for name in list_names(kind, coarse) for t in getattr(model, name)]


def assign(model, kind: str, tensors, coarse: bool = False) -> None:
    """Puts 12 tensors in the canonical order into the model's table lists."""
    it = iter(tensors)
    for name in list_names(kind, coarse):
        for i in range(3):
            getattr(model, name)[i] = next(it)


def shapes_of(tensors):
    return [(t.shape[1], t.shape[2], t.shape[3]) for t in tensors]


def carve_channel_last(shapes, device, dtype=torch.float32) -> List[torch.Tensor]:
    """One flat allocation carved into [1,H,W,C]-memory tables, returned as reference-shaped (1,C,H,W) views.  The tables of a
    field come from one buffer so that the kernels can address every tap as `base + 32-bit byte offset` (csrc/ego_device.h
    DevField; the library rejects a field whose tables span 4 GB or more).  Each table starts on a 256-byte boundary."""
    esz = torch.empty((), dtype=dtype).element_size()
    align = 256 // esz
    offs, total = [], 0
    for (C_, H, W) in shapes:
        offs.append(total)
        total += (C_ * H * W + align - 1) // align * align
    flat = torch.empty(total, device=device, dtype=dtype)
    return [flat[o:o + C_ * H * W].view(1, H, W, C_).permute(0, 3, 1, 2) for o, (C_, H, W) in zip(offs, shapes)]


def is_compact(tensors) -> bool:
    """True iff the tensors end within 4 GB of the lowest of them (what csrc/ego_device.h's 32-bit tap offsets need;
    ego_field_is_compact is the library's own check)."""
    lo = min(t.data_ptr() for t in tensors)
    hi = max(t.data_ptr() + t.numel() * t.element_size() for t in tensors)
    return hi - lo < (1 << 32)


@torch.no_grad()
def recarve(model, kind: str, keep_parameters: bool) -> None:
    """Move the 12 tables of `kind` into one fresh carved buffer.  Needed after anything that re-allocates them one by one: separate
    hipMalloc segments of this size have no bounded distance, and the forward gathers address a tap as base + 32-bit offset.
    keep_parameters=True (after `Module._apply`: .to() / .cuda() / .float(), or `load_state_dict(assign=True)`): in place,
    `param.data = view` - the Parameter objects, and with them an optimiser's references and state, stay.
    keep_parameters=False (after upsample_volume_grid replaced the tables): new Parameters, so an optimiser must be rebuilt
    afterwards (the reference does, train.py:380)."""
    olds = tables(model, kind)
    views = carve_channel_last(shapes_of(olds), olds[0].device)
    for v, p in zip(views, olds):
        v.copy_(p.data)
        if keep_parameters:
            p.data = v
    if not keep_parameters:
        assign(model, kind, [torch.nn.Parameter(v, requires_grad=p.requires_grad) for v, p in zip(views, olds)])
    model.invalidate_scene()


def fill_pointers(field_struct, tensors) -> None:
    """Writes the device pointers of 12 tables in the canonical order into `plane[grid][i]` / `line[grid][i]` of an ego_vm_field,
    after checking that the memory of every (1,C,H,W) table really is [H][W][C]."""
    for t in tensors:
        if t is None:
            raise RuntimeError("coarse density tables missing: call update_coarse_sigma_grid()")
        if not t.permute(0, 2, 3, 1).is_contiguous():
            raise RuntimeError(f"table of shape {tuple(t.shape)} / strides {t.stride()} is not channel-last; "
                               "assign parameters with param.data.copy_(...) so the layout is kept")
    for gi in range(2):
        for i in range(3):
            field_struct.plane[gi][i] = tensors[gi * 6 + i].data_ptr()
            field_struct.line[gi][i] = tensors[gi * 6 + 3 + i].data_ptr()
