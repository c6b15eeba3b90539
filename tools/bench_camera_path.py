"""Frames per second of a camera path: the loop a user writes without egonerf_amd.camera against FrameRenderer.render_path.

    python tools/bench_camera_path.py                      # both workloads, 3 repetitions -> profiles/r09/camera_path.json
    python tools/bench_camera_path.py --workloads pinhole --reps 1 --poses 8

Workloads (a `synth` model of the Ricoh-like field bench.py's `--config erp` renders: full grid, envmap on, 128 + 128 samples), over a
32-pose orbit:  `erp` 1024 x 2048 equirectangular;  `pinhole` 800 x 800, focal 400.
Legs, alternated a / b / c / a / b / c ..., each one a process of its own under its own time limit, each behind a warm-up of two
frames, with a device synchronisation before and after the timed loop:
  a  baseline, API that predates the camera module: erp_rays / torch pinhole rays -> volume_renderer(keep_alpha=False) -> torch
     clamp, * 255, .to(uint8) and the depth index -> .cpu()
  b  FrameRenderer(...).render_path(poses), eager
  c  the same with graph=True
Every leg delivers the same products per frame on the host: rgb8 [H, W, 3] and the 8-bit depth index [H, W].
The first leg that fails or runs out of time ends the run: nothing more is started, what was measured is written, the exit status is 1.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np

WORKLOADS = {"erp": dict(H=1024, W=2048, camera="erp", focal=None), "pinhole": dict(H=800, W=800, camera="pinhole", focal=400.0)}
KW = dict(n_coarse=128, n_fine=128, exp_sampling=True, resampling=True, use_coarse_sample=True)
CHUNK = 16384


def orbit(K: int) -> np.ndarray:
    p = np.zeros((K, 3, 4), np.float32)
    for k in range(K):
        ang = 2 * np.pi * k / K
        c, s = np.cos(ang), np.sin(ang)
        p[k] = [[c, 0, s, 0.3 * c], [0, 1, 0, 0.05 * (k % 5)], [-s, 0, c, 0.3 * s]]
    return p


def run_leg(leg: str, workload: str, n_poses: int, weights_dir: str) -> dict:
    import torch
    from egonerf_amd import synth
    from egonerf_amd.camera import depth_range
    from egonerf_amd.renderer import FrameRenderer, erp_rays, volume_renderer
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig(**synth.RICOH)
    weights = {k[:-4]: np.load(os.path.join(weights_dir, k)) for k in os.listdir(weights_dir) if k.endswith(".npy")}
    model = synth.build_model(cfg, weights, dev)
    w = WORKLOADS[workload]
    H, W, poses = w["H"], w["W"], orbit(n_poses)
    mi, den = (float(v) for v in depth_range(model.near_far))

    if leg == "a":
        if w["camera"] != "erp":   # get_ray_directions + get_rays as torch operations on the device
            j, i = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32) + 0.5, torch.arange(W, device=dev, dtype=torch.float32) + 0.5,
                                  indexing="ij")
            dirs = torch.stack([(i - W / 2) / w["focal"], (j - H / 2) / w["focal"], torch.ones_like(i)], -1).view(-1, 3)

        def frames(ps):
            for p in ps:
                if w["camera"] == "erp":
                    rays = erp_rays(H, W, p, dev)
                else:
                    c2w = torch.from_numpy(p).to(dev)
                    rays = torch.cat([c2w[:, 3].expand(H * W, 3), dirs @ c2w[:, :3].T], 1)
                with torch.no_grad():
                    rgb, depth = volume_renderer(rays, model, chunk=CHUNK, device=dev, keep_alpha=False, **KW)[:2]
                    rgb8 = (rgb.clamp(0.0, 1.0) * 255).to(torch.uint8).view(H, W, 3)
                    idx8 = (255 * ((torch.nan_to_num(depth) - mi) / den)).clamp(0, 255).to(torch.uint8).view(H, W)
                yield rgb8.cpu().numpy(), idx8.cpu().numpy()
    else:
        fr = FrameRenderer(model, H, W, camera=w["camera"], focal=w["focal"], chunk=CHUNK, palette=False, graph=(leg == "c"), **KW)
        frames = fr.render_path

    check = 0
    for f in frames(poses[:2]):   # warm-up
        check += int(f[0][0, 0, 0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in frames(poses):
        check += int(f[0][H // 2, W // 2, 0]) + int(f[1][H // 2, W // 2])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(leg=leg, workload=workload, frames=n_poses, seconds=dt, fps=n_poses / dt, checksum=check)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workloads", nargs="+", default=["erp", "pinhole"], choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--poses", type=int, default=32)
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds per leg (a process of its own)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09", "camera_path.json"))
    ap.add_argument("--leg", choices=["a", "b", "c"], help=argparse.SUPPRESS)      # child mode
    ap.add_argument("--weights", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        print("RESULT " + json.dumps(run_leg(a.leg, a.workloads[0], a.poses, a.weights)), flush=True)
        return 0

    from egonerf_amd import synth
    results, failed = [], None
    with tempfile.TemporaryDirectory() as tmp:
        for k, v in synth.make_weights(synth.SceneConfig(**synth.RICOH), seed=1234).items():   # once: every leg loads the same arrays
            np.save(os.path.join(tmp, k + ".npy"), v)
        for workload in a.workloads:
            for rep in range(a.reps):
                for leg in "abc":
                    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--workloads", workload, "--poses", str(a.poses), "--weights", tmp]
                    try:
                        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
                    except subprocess.TimeoutExpired:
                        failed = f"{workload} leg {leg} repetition {rep}: no result within {a.leg_timeout} s"
                        break
                    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                    if r.returncode != 0 or not line:
                        failed = f"{workload} leg {leg} repetition {rep}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
                        break
                    res = dict(json.loads(line[-1][7:]), rep=rep)
                    results.append(res)
                    print(f"{workload:8s} rep {rep} leg {leg}: {res['fps']:.3f} frames/s ({res['seconds']:.2f} s)", flush=True)
                if failed:
                    break
            if failed:
                break
    med = {}
    for workload in a.workloads:
        for leg in "abc":
            v = [r["fps"] for r in results if r["workload"] == workload and r["leg"] == leg]
            if v:
                med[f"{workload}/{leg}"] = dict(median_fps=float(np.median(v)), min_fps=min(v), max_fps=max(v), n=len(v))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/bench_camera_path.py", poses=a.poses, samples="128+128", chunk=CHUNK, legs=dict(
            a="erp_rays / torch pinhole rays -> volume_renderer -> torch clamp, scale, uint8 -> .cpu()", b="FrameRenderer.render_path, eager",
            c="FrameRenderer.render_path, graph=True"), workloads={k: WORKLOADS[k] for k in a.workloads}, summary=med, runs=results,
            failed=failed), f, indent=1)
        f.write("\n")
    print(json.dumps(med, indent=1))
    if failed:
        print("STOPPED: " + failed, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
