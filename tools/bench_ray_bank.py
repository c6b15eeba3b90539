"""Feeding the graphed training step: the host loop of INTEGRATION.md (host SimpleSampler, `step(allrays[ids], allrgbs[ids])` with
allrays on the device and allrgbs on the host) against `step()` with a DeviceSimpleSampler over a RayBank (the batch drawn inside the
replayed graph).  BASELINE configs[3] shape - 8192 rays x (128 + 128) samples, resampling - on a synthetic bank of 16 images of
1000 x 2000 pixels.  Legs alternate a / b / a / b in one process; each leg is `--warmup` iterations, then `--iters` iterations under a
host clock that ends in one device synchronisation.  A record, not a test:

    python tools/bench_ray_bank.py [--out profiles/r07/ray_bank_feed.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from egonerf_amd import synth  # noqa: E402
from egonerf_amd.data import RayBank  # noqa: E402
from egonerf_amd.optim import FusedAdam  # noqa: E402
from egonerf_amd.sampler import DeviceSimpleSampler, SimpleSampler  # noqa: E402
from egonerf_amd.train import GraphedTrainStep  # noqa: E402

KW = dict(n_coarse=128, n_fine=128, exp_sampling=True, resampling=True, use_coarse_sample=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--height", type=int, default=1000)
    ap.add_argument("--width", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", type=int, default=2, help="legs per variant (alternated)")
    ap.add_argument("--n-voxel", type=float, default=None, help="grid size (default: the shipped 27e6)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07", "ray_bank_feed.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = "cuda"
    K, H, W, N = a.images, a.height, a.width, a.rays
    g = np.random.default_rng(5)
    q, _ = np.linalg.qr(g.standard_normal((K, 3, 3)))
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    poses[:, :3, :3], poses[:, :3, 3] = q, g.uniform(-0.25, 0.25, (K, 3))
    bank = RayBank(poses, g.integers(0, 256, (K, H, W, 4), dtype=np.uint8), (W, H), device=dev)

    # (a)'s arrays, as the reference's dataset holds them: every ray on the device, every colour as float32 on the host
    per = H * W
    allrays = torch.empty(K * per, 6, device=dev)
    allrgbs = torch.empty(K * per, 3)
    for k in range(K):
        r, c = bank.gather(torch.arange(k * per, (k + 1) * per, device=dev))
        allrays[k * per:(k + 1) * per] = r
        allrgbs[k * per:(k + 1) * per] = c.cpu()
    torch.cuda.synchronize()

    def make(**kw):
        cfg = synth.SceneConfig() if not a.n_voxel else synth.SceneConfig(n_voxel=a.n_voxel)
        model = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), dev)
        model.train()
        opt = FusedAdam(model.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=0.1 ** (1 / 30000))
        return GraphedTrainStep(model, opt, render_kwargs=KW, warmup=2, **kw)

    np.random.seed(20221028)
    sampler = SimpleSampler(K * per, N)
    t0 = time.perf_counter()
    ids = sampler.nextids()                       # the epoch's np.random.permutation(total) happens here
    t_perm = time.perf_counter() - t0
    step_a = make(rays=allrays[ids], target=allrgbs[ids].to(dev))
    step_b = make(batch_source=DeviceSimpleSampler(bank, N, seed=20221028))

    def leg_a(n):
        for _ in range(n):
            ids = sampler.nextids()
            step_a(allrays[ids], allrgbs[ids])

    def leg_b(n):
        for _ in range(n):
            step_b()

    def timed(leg):
        leg(a.warmup)
        torch.cuda.synchronize()
        t = time.perf_counter()
        leg(a.iters)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.iters * 1e3

    legs = []
    for _ in range(a.legs):
        legs.append(dict(variant="a_host_loop", ms_per_iteration=timed(leg_a)))
        legs.append(dict(variant="b_device_feed", ms_per_iteration=timed(leg_b)))
    ms = lambda v: [l["ms_per_iteration"] for l in legs if l["variant"] == v]
    out = dict(
        what="graphed training step, 8192 x (128 + 128), fed by (a) host SimpleSampler + step(allrays[ids], allrgbs[ids]) or (b) step() with "
             "DeviceSimpleSampler over a RayBank; host clock around each leg, one device synchronisation at its end, profiler off",
        shape=dict(rays=N, images=K, height=H, width=W, iters=a.iters, warmup=a.warmup, n_voxel=a.n_voxel or 27e6, **KW),
        legs=legs,
        a_ms=ms("a_host_loop"), b_ms=ms("b_device_feed"),
        a_spread_ms=max(ms("a_host_loop")) - min(ms("a_host_loop")),
        b_not_slower_than_a_beyond_a_spread=max(ms("b_device_feed")) <= max(ms("a_host_loop")) + (max(ms("a_host_loop")) - min(ms("a_host_loop"))),
        a_holds=dict(device_bytes=allrays.numel() * 4, host_bytes=allrgbs.numel() * 4 + K * per * 8,
                     note="all_rays float32 on the device; all_rgbs float32 + the epoch's int64 permutation on the host"),
        b_holds=dict(device_bytes=bank.nbytes, host_bytes=0),
        a_first_nextids_s=t_perm,
        a_note="every (a) leg runs inside ONE permutation epoch: np.random.permutation(total) (a_first_nextids_s, once per "
               f"{K * per // N} iterations) is outside the timed windows",
        device=torch.cuda.get_device_name(0),
    )
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
