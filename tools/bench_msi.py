"""Multi-sphere images on the Ricoh-like synthetic field at 128 samples: bake time, playback against the direct render, fidelity.

    python tools/bench_msi.py                     # L = 16, 32, 64 -> profiles/r11/msi.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_msi.py --child --L 32 --reps 1 --cams erp --big-chunk 0
    python tools/bench_msi.py --trace DIR --L 32  # the two MSI kernels in that trace: time per launch, bytes per second of the taps asked for

The model is bench_camera_path.py's (`synth.RICOH`: full grid, envmap on).  One step = one process = one L, under a time limit of its own:
it bakes an Hm x Wm image with half texels (timed between device synchronisations, after a warm-up bake of one chunk's worth), then times
`FrameRenderer(msi)` against `FrameRenderer(model, n_coarse=128, exp_sampling=True)` - the direct render of the same integral, the path
that exists without this module - for a 1024 x 2048 equirectangular frame and an 800 x 800 pinhole frame, both in chunks of 16384 pixels,
and `FrameRenderer(msi, chunk=262144)` (the `_big` legs: launches that fill the device): all six legs in the same
process, alternated, `frames` frames per leg and repetition, the median over repetitions reported.  Last, the PSNR of the MSI's 8-bit
frame against the direct render's at the same pose (identity rotation, the eye moved along +x by 0, 5, 10 and 20 % of the innermost
radius).  The first step that fails or runs out of time ends the run: nothing more is started, what was measured is written, the exit
status is 1.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERP, PIN, FOCAL, CHUNK, S = (1024, 2048), (800, 800), 700.0, 16384, 128
BIG_CHUNK = 262144   # a playback launch of 16384 rays is 256 waves, one per compute unit: the `_big` legs give the kernel 16 x as many
OFFSETS = (0.0, 0.05, 0.10, 0.20)
DIRECT = dict(n_coarse=S, exp_sampling=True)
OUR_KERNELS = re.compile(r"k_msi_(render|layers)")


def pose_at(centre, dx: float) -> np.ndarray:
    p = np.concatenate([np.eye(3, dtype=np.float32), np.asarray(centre, np.float32).reshape(3, 1)], axis=1)
    p[0, 3] += dx
    return p


def psnr8(a, b):
    """PSNR in dB of two uint8 images (peak 255); None when they are identical."""
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return None if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


def run_step(L: int, Hm: int, Wm: int, reps: int, frames: int, cam_names=("erp", "pinhole"), msi_chunk: int = CHUNK, big_chunk: int = BIG_CHUNK) -> dict:
    import torch
    from egonerf_amd import synth
    from egonerf_amd.camera import FrameRenderer
    from egonerf_amd.msi import bake_msi
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig(**synth.RICOH)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), dev)
    bake_msi(model, 64, 256, L, S, chunk=CHUNK)   # warm-up: code objects, the scene and schedule caches, the allocator's blocks
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    msi = bake_msi(model, Hm, Wm, L, S, chunk=CHUNK)
    torch.cuda.synchronize()
    out = dict(L=L, msi=[Hm, Wm], texel="float16", bake_seconds=time.perf_counter() - t0,
               image_mbytes=msi.layers.numel() * 2 / 1e6, innermost_radius=float(msi.radii[0]), outermost_radius=float(msi.radii[-1]))
    cams = {"erp": dict(H=ERP[0], W=ERP[1], camera="erp"), "pinhole": dict(H=PIN[0], W=PIN[1], camera="pinhole", focal=FOCAL)}
    legs = {}
    for cam in cam_names:
        kw = cams[cam]
        legs[f"msi_{cam}"] = FrameRenderer(msi, chunk=msi_chunk, palette=False, **kw)
        legs[f"direct_{cam}"] = FrameRenderer(model, chunk=CHUNK, palette=False, **kw, **DIRECT)
        if big_chunk:
            legs[f"msi_{cam}_big"] = FrameRenderer(msi, chunk=big_chunk, palette=False, **kw)
    pose = pose_at(msi.center, 0.05 * float(msi.radii[0]))
    check = 0
    for fr in legs.values():   # warm-up of every shape the timed window uses
        check += int(fr.render(pose)[0][0, 0, 0])
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for name, fr in legs.items():
            t0 = time.perf_counter()
            for _ in range(frames):
                img = fr.render(pose)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / frames * 1e3)
            check += int(img[0][0, 0, 0])
    out["ms_per_frame"] = {k: dict(median=float(np.median(v)), min=min(v), max=max(v), n=len(v)) for k, v in times.items()}
    out["psnr_db"] = {}
    for frac in OFFSETS if "erp" in cam_names else ():
        p = pose_at(msi.center, frac * float(msi.radii[0]))
        a, b = legs["msi_erp"].render(p)[0].cpu().numpy(), legs["direct_erp"].render(p)[0].cpu().numpy()
        out["psnr_db"][f"{frac:.2f}"] = psnr8(a, b)
    out["checksum"] = check
    return out


def trace_summary(directory: str, L: int, chunk: int = CHUNK) -> dict:
    """The two MSI kernels in a `rocprofv3 --kernel-trace --stats` run of `--child --L L`: calls, total and mean time, and for k_msi_render
    the rate at which its taps were asked for: launches x `chunk` rays x L layers x 4 taps x the texel's bytes over the kernel's time.  Every
    launch is counted as a full chunk, which holds for a run with `--cams erp --big-chunk 0` (a 1024 x 2048 frame is whole chunks; the last
    chunk of a pinhole frame is shorter); a skipped layer and the background's tap are not counted; the taps are served by the caches, so this is a request rate, not HBM traffic."""
    stats = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    dbs = sorted(glob.glob(os.path.join(directory, "**", "*.db"), recursive=True))
    if stats:
        src = stats[-1]
        with open(src, newline="") as f:
            table = [(r.get("Name", ""), int(r.get("Calls", 0) or 0), float(r.get("TotalDurationNs", 0) or 0)) for r in csv.DictReader(f)]
    elif dbs:
        import sqlite3
        src = dbs[-1]
        table = sqlite3.connect(src).execute("select name, count(*), sum(end - start) from kernels group by name").fetchall()
    else:
        raise SystemExit(f"neither *kernel_stats.csv nor a rocpd *.db under {directory}")
    rows, total = {}, 0.0
    for name, calls, ns in table:
        total += ns
        m = OUR_KERNELS.search(name)
        if m:
            half = "Float16" in name or "DF16_" in name
            row = dict(calls=calls, total_ms=ns / 1e6, mean_us=ns / 1e3 / max(calls, 1))
            if m.group(1) == "render" and ns > 0 and chunk:
                row["ns_per_ray_and_layer"] = ns / (calls * chunk * L)
                row["tap_gbytes_per_s"] = calls * chunk * L * 4 * (8 if half else 16) / ns
            rows[m.group(0) + ("<half>" if half else "<float>")] = row
    return dict(source=os.path.basename(src), L=L, chunk=chunk, kernel_time_ms=total / 1e6, kernels=rows)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--L", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--msi", type=int, nargs=2, default=[1024, 2048], metavar=("HM", "WM"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per step (a process of its own)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r11", "msi.json"))
    ap.add_argument("--trace", help="summarise the kernel statistics of a rocprofv3 run in this directory (into --out, key `trace`) and exit")
    ap.add_argument("--cams", nargs="+", default=["erp", "pinhole"], choices=["erp", "pinhole"], help="--child: the frames to time")
    ap.add_argument("--msi-chunk", type=int, default=CHUNK, help="--child: pixels per playback launch of the msi_* legs; --trace: what that run used")
    ap.add_argument("--big-chunk", type=int, default=BIG_CHUNK, help="--child: pixels per playback launch of the msi_*_big legs (0: none)")
    ap.add_argument("--trace-key", default="trace", help="--trace: the key of --out that takes the summary")
    ap.add_argument("--child", action="store_true", help="run one step (the first --L) in this process and print the result")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, HERE)
        print("RESULT " + json.dumps(run_step(a.L[0], a.msi[0], a.msi[1], a.reps, a.frames, a.cams, a.msi_chunk, a.big_chunk)), flush=True)
        return 0
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.trace:
        doc[a.trace_key] = trace_summary(a.trace, a.L[0], a.msi_chunk)
        print(json.dumps(doc[a.trace_key], indent=1))
    else:
        steps, failed = [], None
        for L in a.L:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--L", str(L), "--msi", str(a.msi[0]), str(a.msi[1]),
                   "--reps", str(a.reps), "--frames", str(a.frames)]
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
            ms = res["ms_per_frame"]
            print(f"L {L:3d}: bake {res['bake_seconds']:.2f} s; erp {ms['msi_erp']['median']:.2f} vs {ms['direct_erp']['median']:.2f} ms; "
                  f"pinhole {ms['msi_pinhole']['median']:.2f} vs {ms['direct_pinhole']['median']:.2f} ms; chunks of {BIG_CHUNK}: erp "
                  f"{ms['msi_erp_big']['median']:.2f}, pinhole {ms['msi_pinhole_big']['median']:.2f} ms; psnr {res['psnr_db']}", flush=True)
        doc.update(tool="tools/bench_msi.py", samples=S, direct=DIRECT, frames_erp=list(ERP), frames_pinhole=list(PIN), focal=FOCAL, chunk=CHUNK, big_chunk=BIG_CHUNK,
                   offsets_of_innermost_radius=list(OFFSETS), reps=a.reps, frames_per_rep=a.frames, steps=steps, failed=failed)
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
