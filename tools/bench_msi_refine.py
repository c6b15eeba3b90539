"""Differentiable playback and texel refinement of multi-sphere images on the Ricoh-like synthetic field at 128 samples.

    python tools/bench_msi_refine.py                     # L = 16, 32 -> profiles/r13/msi_refine.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_msi_refine.py --child --L 32 --only times
    python tools/bench_msi_refine.py --trace DIR --L 32  # the playback kernels in that trace, into the JSON under `trace`
    python tools/bench_msi_refine.py --optimizer texel   # the texel optimiser next to the dense one -> profiles/r16/msi_texel_adam.json

The model, the bake (1024 x 2048, half texels), the frames and the PSNR are tools/bench_msi.py's: the `before` column repeats
profiles/r11/msi.json's method.  One step = one process = one L, under a time limit of its own.
(a) Times of one refinement step's parts at `--rays` rays drawn from the headbox, each between device synchronisations, the legs
    alternated, the median over repetitions: the teacher's render, playback forward, playback backward (`backward_quad`: four lanes
    add the four channels of a texel; into gradient buffers that are not re-zeroed: the adds do not depend on what they add to),
    zeroing the gradient, FusedAdam, the projection.  profiles/r13/msi_refine.json also holds `removed_thread_per_ray`: the times of
    the mapping that was built first, measured by this tool next to the kept one and then removed as the slower of the two; the tool
    keeps every key of an existing record that it does not write itself.
    The backward against two yardsticks: the forward on the same rays, and the atomic floor (added bytes over 1.3 TB/s; every layer is
    live inside the headbox, so a ray adds 64 B per layer and 48 B to the background - an add of exactly 0 is skipped, so this is an
    upper count).
(b) PSNR of the 8-bit 1024 x 2048 ERP frame against the direct render's at eye offsets of 0, 5, 10 and 20 % of the innermost radius,
    before and after `refine_msi` with headbox = 0.2 x the innermost radius, for every learning rate of the sweep; same poses.
`--optimizer texel` (the default `dense` is the record above, unchanged) measures `refine_msi(optimizer="texel")` against the dense loop
in the same run.  (a) gains legs: `backward_texel_step`, the backward into persistent gradient buffers followed by the fused
ego_msi_adam_step that projects and re-zeroes (the step consumes its gradient, so it cannot be repeated without a backward; the fused
step's time is this leg minus `backward_quad`, and it stands against `zero_grad` + `adam` + `project`); `texel_step_keep_grad`, the
fused step without re-zeroing on a gradient that stays (a lower bound: it lacks the 16-byte store per touched texel); `step_dense` and
`step_texel`, one whole iteration of either loop, teacher included; and `touched_share`, the share of texels with a non-zero gradient
after one backward.  (b) runs `texel` at `--lrs` (default 1e-3, 3e-4, 1e-4, 3e-5) and `dense` at `--dense-lrs` (default 1e-3, 3e-5).
The first step that fails or runs out of time ends the run: nothing more is started, what was measured is written, the exit status is 1."""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_msi import CHUNK, DIRECT, ERP, OFFSETS, S, pose_at, psnr8   # noqa: E402

ATOMIC_RATE = 1.3e12   # bytes of float atomic adds per second, chip-wide
LRS = (1e-3, 3e-3, 1e-2, 1e-4, 3e-5, 1e-5)   # the three rates the default was to be chosen from, then the sweep continued downwards
TEXEL_LRS, DENSE_LRS_BESIDE_TEXEL = (1e-3, 3e-4, 1e-4, 3e-5), (1e-3, 3e-5)
OUR_KERNELS = re.compile(r"k_msi_(render_bwd\w*|render|project|adam)")


def time_legs(legs: dict, reps: int, iters: int) -> dict:
    import torch
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / iters * 1e3)
    return {k: dict(median=float(np.median(v)), min=min(v), max=max(v), n=len(v)) for k, v in times.items()}


def texel_legs(msi, model, work, rays, backward, headbox: float, rays_per_step: int) -> tuple:
    """The legs `--optimizer texel` adds (module docstring) and the share of texels one backward touches."""
    import torch
    from egonerf_amd.msi import MultiSphereImage, headbox_rays, project_msi
    from egonerf_amd.optim import FusedAdam, TexelAdam
    dev = rays.device

    def copy_of(image, requires_grad):
        bg = None if image.background is None else image.background.detach().clone().requires_grad_(requires_grad)
        return MultiSphereImage(image.layers.detach().clone().requires_grad_(requires_grad), msi.radii, msi.bounds, msi.center, msi.near_far, bg)

    params = list(work.parameters())   # their .grad are the buffers `backward` adds into
    for g in (p.grad for p in params):
        g.zero_()
    backward()
    touched = sum(int((p.grad != 0).any(dim=-1).sum()) for p in params) / sum(p.numel() // 4 for p in params)
    fused = TexelAdam(params, lr=1e-3, project=True, zero_grad=True)
    kept = TexelAdam(params, lr=1e-3, project=True, zero_grad=False)
    center = torch.from_numpy(msi.center).to(dev)
    gen = torch.Generator(device=dev).manual_seed(2)
    # one whole iteration of either loop, as refine_msi runs it
    dense_work = copy_of(work, True)
    dense_opt = FusedAdam(list(dense_work.parameters()), lr=1e-5, betas=(0.9, 0.99))
    texel_work = copy_of(work, False)
    for p in texel_work.parameters():
        p.grad = torch.zeros_like(p)
    texel_opt = TexelAdam(list(texel_work.parameters()), lr=1e-5, project=True, zero_grad=True)
    texel_bg_grad = None if texel_work.background is None else texel_work.background.grad

    def step_dense():
        r = headbox_rays(rays_per_step, center, headbox, gen)
        with torch.no_grad():
            target = model(r, is_train=False, need_alpha=False, **DIRECT)[0]
        with torch.enable_grad():
            loss = torch.mean((dense_work.render(r)[0] - target) ** 2)
            loss.backward()
        dense_opt.step()
        dense_opt.zero_grad()
        project_msi(dense_work)

    def step_texel():
        with torch.no_grad():
            r = headbox_rays(rays_per_step, center, headbox, gen)
            target = model(r, is_train=False, need_alpha=False, **DIRECT)[0]
            diff = texel_work._render(r, texel_work.layers, texel_work.background)[0] - target
            texel_work._render_backward(r, texel_work.layers, texel_work.background, diff * (2.0 / (3 * rays_per_step)), texel_work.layers.grad,
                                        texel_bg_grad)
            texel_opt.step()
            torch.mean(diff ** 2)

    def backward_texel_step():
        backward()
        fused.step()

    def refill():   # what `backward_texel_step` left zero, for the leg whose gradient stays
        backward()

    return dict(backward_texel_step=backward_texel_step, texel_step_keep_grad=kept.step, step_dense=step_dense, step_texel=step_texel), touched, refill


def run_step(L: int, Hm: int, Wm: int, rays_per_step: int, steps: int, lrs, reps: int, iters: int, only: str, optimizer: str = "dense",
             dense_lrs=()) -> dict:
    import torch
    from egonerf_amd import synth
    from egonerf_amd.camera import FrameRenderer
    from egonerf_amd.msi import MultiSphereImage, bake_msi, headbox_rays, project_msi, refine_msi
    from egonerf_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig(**synth.RICOH)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), dev)
    msi = bake_msi(model, Hm, Wm, L, S, chunk=CHUNK)
    r0 = float(msi.radii[0])
    headbox = 0.2 * r0
    out = dict(L=L, msi=[Hm, Wm], texel="float16", innermost_radius=r0, headbox=headbox, rays_per_step=rays_per_step)
    if only in ("all", "times"):
        work = msi.float()
        work = MultiSphereImage(work.layers.clone().requires_grad_(True), msi.radii, msi.bounds, msi.center, msi.near_far,
                                None if work.background is None else work.background.clone().requires_grad_(True))
        rays = headbox_rays(rays_per_step, torch.from_numpy(msi.center).to(dev), headbox, torch.Generator(device=dev).manual_seed(1))
        g_rgb = torch.randn(rays_per_step, 3, device=dev) / rays_per_step
        params = list(work.parameters())
        grads = [torch.zeros_like(p) for p in params]
        g_bg = grads[1] if len(grads) > 1 else None
        for p, g in zip(params, grads):
            p.grad = g
        opt = FusedAdam(params, lr=1e-3, betas=(0.9, 0.99))

        def backward():
            with torch.no_grad():
                work._render_backward(rays, work.layers, work.background, g_rgb, grads[0], g_bg)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run

        legs = dict(teacher=no_grad(lambda: model(rays, is_train=False, need_alpha=False, **DIRECT)),
                    forward=no_grad(lambda: work.render(rays)),
                    backward_quad=backward,
                    zero_grad=no_grad(lambda: [g.zero_() for g in grads]), adam=opt.step, project=lambda: project_msi(work))
        if optimizer == "texel":
            more, out["touched_share"], refill = texel_legs(msi, model, work, rays, backward, headbox, rays_per_step)
            legs.update(more)
            keep = legs.pop("texel_step_keep_grad")   # in a pass of its own: the other legs zero or overwrite the gradient it needs
        ms = time_legs(legs, reps, iters)
        if optimizer == "texel":
            for g in grads:
                g.zero_()
            refill()
            ms.update(time_legs(dict(texel_step_keep_grad=keep), reps, iters))
            dense_sum = ms["zero_grad"]["median"] + ms["adam"]["median"] + ms["project"]["median"]
            fused_ms = ms["backward_texel_step"]["median"] - ms["backward_quad"]["median"]
            out["dense_update_ms"], out["fused_update_ms"] = dense_sum, fused_ms
            out["fused_update_spread_ms"] = sum(ms[k]["max"] - ms[k]["min"] for k in ("backward_texel_step", "backward_quad"))   # of a difference
            out["dense_update_spread_ms"] = sum(ms[k]["max"] - ms[k]["min"] for k in ("zero_grad", "adam", "project"))
            del more, keep, refill
        legs.clear()
        added = rays_per_step * (L * 64 + (48 if g_bg is not None else 0))
        floor_ms = added / ATOMIC_RATE * 1e3
        out["ms_per_step_part"] = ms
        out["backward_added_bytes"], out["atomic_floor_ms"] = added, floor_ms
        out["backward_over_forward"] = {"backward_quad": ms["backward_quad"]["median"] / ms["forward"]["median"]}
        out["backward_over_atomic_floor"] = {"backward_quad": ms["backward_quad"]["median"] / floor_ms}
        del work, grads, opt, params
        torch.cuda.empty_cache()
    if only in ("all", "quality"):
        kw = dict(H=ERP[0], W=ERP[1], camera="erp")
        direct = FrameRenderer(model, chunk=CHUNK, palette=False, **kw, **DIRECT)
        poses = {f"{frac:.2f}": pose_at(msi.center, frac * r0) for frac in OFFSETS}
        want = {k: direct.render(p)[0].cpu().numpy() for k, p in poses.items()}

        def psnr(image):
            fr = FrameRenderer(image, chunk=CHUNK, palette=False, **kw)
            return {k: psnr8(fr.render(p)[0].cpu().numpy(), want[k]) for k, p in poses.items()}

        out["psnr_db_before"] = psnr(msi)
        out["refined"] = []
        runs = [(optimizer, lr) for lr in lrs] + ([("dense", lr) for lr in dense_lrs] if optimizer == "texel" else [])
        for which, lr in runs:
            log = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            extra = dict(optimizer=which) if optimizer == "texel" else {}   # the default call is the r13 record's, as it was
            refined = refine_msi(msi, model, steps, rays_per_step=rays_per_step, headbox=headbox, lr=lr, seed=0, render_kwargs=DIRECT, log=log,
                                 **extra)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            losses = torch.stack(log).cpu().numpy() if log else np.zeros(0)
            k = max(1, len(losses) // 20)
            out["refined"].append(dict(**extra, lr=lr, steps=steps, ms_per_step=wall / max(steps, 1) * 1e3, psnr_db=psnr(refined),
                                       loss_first=float(losses[:k].mean()) if len(losses) else None,
                                       loss_last=float(losses[-k:].mean()) if len(losses) else None))
            del refined
            torch.cuda.empty_cache()
    return out


def trace_summary(directory: str, L: int, rays_per_step: int) -> dict:
    """The playback kernels in a `rocprofv3 --kernel-trace --stats` run of `--child --L L --only times`: calls, total and mean time,
    and for the backward kernels the rate of added bytes (the upper count of (a))."""
    dbs = sorted(glob.glob(os.path.join(directory, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no rocpd *.db under {directory}")
    import sqlite3
    table = sqlite3.connect(dbs[-1]).execute("select name, count(*), sum(end - start) from kernels group by name").fetchall()
    rows = {}
    for name, calls, ns in table:
        m = OUR_KERNELS.search(name)
        if m and calls:
            key = m.group(0) + ("<half>" if ("Float16" in name or "DF16_" in name) else "")
            row = dict(calls=calls, total_ms=ns / 1e6, mean_us=ns / 1e3 / calls)
            if "bwd" in key and ns > 0:
                row["added_gbytes_per_s"] = calls * rays_per_step * (L * 64 + 48) / ns
            rows[key] = row
    return dict(L=L, rays_per_step=rays_per_step, kernels=rows)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--L", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--msi", type=int, nargs=2, default=[1024, 2048], metavar=("HM", "WM"))
    ap.add_argument("--rays", type=int, default=65536, help="rays per refinement step")
    ap.add_argument("--steps", type=int, default=1000, help="refinement steps per learning rate")
    ap.add_argument("--lrs", type=float, nargs="+", help=f"default: {LRS}, with --optimizer texel {TEXEL_LRS}")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="calls per leg and repetition")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds per step (a process of its own)")
    ap.add_argument("--optimizer", default="dense", choices=["dense", "texel"],
                    help="dense: today's loop, the r13 record; texel: refine_msi(optimizer='texel') next to the dense loop in one run")
    ap.add_argument("--dense-lrs", type=float, nargs="+", default=list(DENSE_LRS_BESIDE_TEXEL), help="with --optimizer texel: the dense loop's rates")
    ap.add_argument("--out", help="default: profiles/r13/msi_refine.json, with --optimizer texel profiles/r16/msi_texel_adam.json")
    ap.add_argument("--only", default="all", choices=["all", "times", "quality"], help="the part to run: (a) times, (b) quality, or both")
    ap.add_argument("--trace", help="summarise the kernel statistics of a rocprofv3 run in this directory (into --out, key `trace`) and exit")
    ap.add_argument("--child", action="store_true", help="run one step (the first --L) in this process and print the result")
    a = ap.parse_args()
    texel = a.optimizer == "texel"
    a.lrs = a.lrs or list(TEXEL_LRS if texel else LRS)
    a.out = a.out or os.path.join(HERE, "profiles", *(("r16", "msi_texel_adam.json") if texel else ("r13", "msi_refine.json")))
    if a.child:
        sys.path.insert(0, HERE)
        print("RESULT " + json.dumps(run_step(a.L[0], a.msi[0], a.msi[1], a.rays, a.steps, a.lrs, a.reps, a.iters, a.only,
                                                  a.optimizer, a.dense_lrs)), flush=True)
        return 0
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.trace:
        doc["trace"] = trace_summary(a.trace, a.L[0], a.rays)
        print(json.dumps(doc["trace"], indent=1))
    else:
        steps, failed = [], None
        for L in a.L:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--L", str(L), "--msi", str(a.msi[0]), str(a.msi[1]), "--rays", str(a.rays),
                   "--steps", str(a.steps), "--reps", str(a.reps), "--iters", str(a.iters), "--only", a.only, "--lrs", *[repr(v) for v in a.lrs]]
            if texel:
                cmd += ["--optimizer", "texel", "--dense-lrs", *[repr(v) for v in a.dense_lrs]]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                failed = f"L = {L}: no result within {a.step_timeout} s"
                break
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                failed = f"L = {L}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
                break
            res = json.loads(line[-1][7:])
            steps.append(res)
            if "ms_per_step_part" in res:
                ms = {k: round(v["median"], 3) for k, v in res["ms_per_step_part"].items()}
                print(f"L {L:3d}: ms {ms}; atomic floor {res['atomic_floor_ms']:.3f} ms", flush=True)
            if "touched_share" in res:
                print(f"L {L:3d}: touched share {res['touched_share']:.4f}; update: dense {res['dense_update_ms']:.3f} ms "
                      f"(spread {res['dense_update_spread_ms']:.3f}), fused {res['fused_update_ms']:.3f} ms (spread {res['fused_update_spread_ms']:.3f})",
                      flush=True)
            if "psnr_db_before" in res:
                print(f"L {L:3d}: psnr before {res['psnr_db_before']}", flush=True)
            for row in res.get("refined", []):
                print(f"       {row.get('optimizer', 'dense')} lr {row['lr']:g}, {row['steps']} steps ({row['ms_per_step']:.2f} ms each): psnr {row['psnr_db']}; "
                      f"loss {row['loss_first']:.3e} -> {row['loss_last']:.3e}", flush=True)
        moved = [k for k in (f"{f:.2f}" for f in OFFSETS) if k != "0.00"]
        runs = [("dense", lr) for lr in a.lrs] if not texel else [("texel", lr) for lr in a.lrs] + [("dense", lr) for lr in a.dense_lrs]
        gain = {(f"{which} " if texel else "") + repr(lr): float(np.mean([row["psnr_db"][k] - res["psnr_db_before"][k] for res in steps
                                                                         for row in res["refined"]
                                                                         if row["lr"] == lr and row.get("optimizer", "dense") == which for k in moved]))
                for which, lr in runs} if steps and a.only != "times" else {}
        doc.update(tool="tools/bench_msi_refine.py", samples=S, direct=DIRECT, frame_erp=list(ERP), chunk=CHUNK,
                   offsets_of_innermost_radius=list(OFFSETS), atomic_rate_bytes_per_s=ATOMIC_RATE, reps=a.reps, calls_per_rep=a.iters, failed=failed)
        doc.update(steps=steps, mean_psnr_gain_db_off_centre=gain)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not a.trace and doc.get("failed"):
        print("STOPPED: " + doc["failed"], file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
