"""Seconds per frame of a 1024 x 2048 panorama: mono, top-bottom stereo, and 2 x 2 supersampled.

    python tools/bench_vr_frame.py                          # three legs, 3 repetitions -> profiles/r10/vr_frame.json
    python tools/bench_vr_frame.py --legs mono --repo OTHER_TREE --out other.json     # the mono leg of another checkout (the parent commit)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_vr_frame.py --child --legs top_bottom_ss2 --poses 2
    python tools/bench_vr_frame.py --trace DIR              # the ray and resolve kernels' share of that trace's kernel time

The model is bench_camera_path.py's (a `synth` model of the Ricoh-like field: full grid, envmap on, 128 + 128 samples), the path its orbit.
Legs: `mono` FrameRenderer(H, W); `top_bottom` stereo="top_bottom", ipd=0.065; `ss2` supersample=2; `top_bottom_ss2` both (for the
trace).  All eager, palette=False, through render_path, so every frame ends in pinned host memory.  One repetition = one process that
runs the legs one after the other, each behind a warm-up frame, with a device synchronisation before and after the timed loop; the
repetitions alternate the legs a / b / c / a / b / c.  The first repetition that fails or runs out of time ends the run: nothing more is
started, what was measured is written, the exit status is 1.
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
H, W, CHUNK, IPD = 1024, 2048, 16384, 0.065
KW = dict(n_coarse=128, n_fine=128, exp_sampling=True, resampling=True, use_coarse_sample=True)
LEGS = {"mono": {}, "top_bottom": dict(stereo="top_bottom", ipd=IPD), "ss2": dict(supersample=2),
        "top_bottom_ss2": dict(stereo="top_bottom", ipd=IPD, supersample=2)}
OUR_KERNELS = re.compile(r"k_(camera_rays_ex|camera_rays|resolve_frame|finish_frame)(<\d+>)?")   # the two ends of a frame


def orbit(K: int) -> np.ndarray:
    p = np.zeros((K, 3, 4), np.float32)
    for k in range(K):
        ang = 2 * np.pi * k / K
        c, s = np.cos(ang), np.sin(ang)
        p[k] = [[c, 0, s, 0.3 * c], [0, 1, 0, 0.05 * (k % 5)], [-s, 0, c, 0.3 * s]]
    return p


def run_legs(legs, n_poses: int) -> list:
    import torch
    from egonerf_amd import synth
    from egonerf_amd.camera import FrameRenderer
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig(**synth.RICOH)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), dev)
    poses, out = orbit(n_poses), []
    for leg in legs:
        fr = FrameRenderer(model, H, W, chunk=CHUNK, palette=False, **LEGS[leg], **KW)
        check = 0
        for f in fr.render_path(poses[:1]):   # warm-up
            check += int(f[0][0, 0, 0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in fr.render_path(poses):
            check += int(f[0][f[0].shape[0] // 2, W // 2, 0]) + int(f[1][f[1].shape[0] // 2, W // 2])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out.append(dict(leg=leg, frames=n_poses, seconds=dt, seconds_per_frame=dt / n_poses, checksum=check))
        del fr
    return out


def trace_share(directory: str) -> dict:
    """The share of the ray, finish and resolve kernels in the kernel time of a `rocprofv3 --kernel-trace --stats` run: from its
    `*kernel_stats.csv` (--output-format csv) or, failing that, from the `kernels` view of its rocpd database (the default format)."""
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
    total, ours, rows = 0.0, 0.0, {}
    for name, calls, ns in table:
        total += ns
        m = OUR_KERNELS.search(name)
        if m:
            ours += ns
            rows[m.group(0)] = dict(calls=calls, total_ms=ns / 1e6)
    return dict(source=os.path.basename(src), kernel_time_ms=total / 1e6, ray_and_resolve_ms=ours / 1e6,
                share=ours / total if total else None, kernels=rows)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", nargs="+", default=["mono", "top_bottom", "ss2"], choices=sorted(LEGS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--poses", type=int, default=6)
    ap.add_argument("--rep-timeout", type=int, default=240, help="seconds per repetition (a process of its own)")
    ap.add_argument("--repo", default=HERE, help="the checkout whose egonerf_amd is measured (default: this one)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r10", "vr_frame.json"))
    ap.add_argument("--trace", help="summarise the kernel statistics of a rocprofv3 run in this directory (into --out, key `trace`) and exit")
    ap.add_argument("--child", action="store_true", help="run the legs once in this process and print the result")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.abspath(a.repo))
        print("RESULT " + json.dumps(run_legs(a.legs, a.poses)), flush=True)
        return 0
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.trace:
        doc["trace"] = trace_share(a.trace)
        print(json.dumps(doc["trace"], indent=1))
    else:
        results, failed = [], None
        for rep in range(a.reps):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repo", a.repo, "--poses", str(a.poses), "--legs", *a.legs]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.rep_timeout)
            except subprocess.TimeoutExpired:
                failed = f"repetition {rep}: no result within {a.rep_timeout} s"
                break
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                failed = f"repetition {rep}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
                break
            for res in json.loads(line[-1][7:]):
                results.append(dict(res, rep=rep))
                print(f"rep {rep} {res['leg']:15s}: {res['seconds_per_frame'] * 1e3:8.1f} ms / frame", flush=True)
        med = {}
        for leg in a.legs:
            v = [r["seconds_per_frame"] for r in results if r["leg"] == leg]
            if v:
                med[leg] = dict(median_ms=float(np.median(v)) * 1e3, min_ms=min(v) * 1e3, max_ms=max(v) * 1e3, n=len(v))
        for leg in med:
            if "mono" in med:
                med[leg]["times_mono"] = med[leg]["median_ms"] / med["mono"]["median_ms"]
        doc.update(tool="tools/bench_vr_frame.py", frame=[H, W], poses=a.poses, samples="128+128", chunk=CHUNK, ipd=IPD,
                   legs={k: LEGS[k] for k in a.legs}, summary=med, runs=results, failed=failed)
        print(json.dumps(med, indent=1))
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
