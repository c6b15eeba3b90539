"""What the ray gradients cost on the device: the eager training step with and without them, the new kernels alone
next to the forward's own gathers, and a frozen-model localisation step.

    python tools/bench_pose_refine.py            # -> profiles/r17/ray_grad.json

BASELINE configs[3]'s shape, 8192 rays x (128 + 128) samples on the headline scene (bench.py --config train), one process:
(a) step: the eager iteration (render, MSE, backward, FusedAdam, coarse-table refresh) with rays that ask for nothing - the code path
    of the commit before the ray gradients - and with rays.requires_grad; and a localisation step on a frozen model (PoseDeltas over 8
    images -> render -> MSE -> backward -> Adam on the deltas).  One model per leg, the legs alternated, `steps` iterations between two
    device synchronisations, the median over repetitions.
(b) kernels: one stream (train.SIDE_STREAM_SCATTER off), an event behind every library call of a step with ray gradients
    (train.KERNEL_MARKS): the interval in front of a mark is that call's kernel plus the torch glue queued before it.  ego_ray_grad
    re-reads the 36 taps per sample that the fine march (density, 18) and the shade (appearance, 18) read, so those two are its
    yardstick, from the same steps.  The median over repetitions per call name (ego_march_density: the coarse and the fine pass apart).
Nothing here has a pass bar.  Without a device the tool fails; it has no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
RAYS, NC, NF, K_IMAGES = 8192, 128, 128, 8


def summary(v) -> dict:
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), n=len(v))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10, help="iterations per leg and repetition")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r17", "ray_grad.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("tools/bench_pose_refine.py needs a HIP device: a time from anything else says nothing", file=sys.stderr)
        return 1
    from egonerf_amd import synth, train
    from egonerf_amd.optim import FusedAdam
    from egonerf_amd.poses import PoseDeltas
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig()
    weights = synth.make_weights(cfg, seed=1234)
    rays = torch.from_numpy(synth.make_rays(RAYS, seed=1)).to(dev)
    gt = torch.from_numpy(synth.hash_uniform(3, 0, RAYS * 3).reshape(RAYS, 3).astype(np.float32)).to(dev)
    img = torch.from_numpy((synth.hash_uniform(4, 0, RAYS) * K_IMAGES).astype(np.int64)).to(dev)
    kw = dict(is_train=True, n_coarse=NC, n_fine=NF, exp_sampling=True, resampling=True, use_coarse_sample=True)

    def make_leg(leg):
        model = synth.build_model(cfg, weights, dev)
        model.train()
        if leg == "localise_frozen":
            for p in model.parameters():
                p.requires_grad_(False)
            deltas = PoseDeltas(K_IMAGES, device=dev)
            opt = torch.optim.Adam([dict(params=[deltas.rot], lr=1e-3), dict(params=[deltas.trans], lr=1e-3)])
        else:
            opt = FusedAdam(model.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=0.1 ** (1 / 30000))

        def step():
            if leg == "localise_frozen":
                r = deltas.apply(rays, img)
            else:
                r = rays.clone().requires_grad_(True) if leg == "train_ray_grads" else rays
            rgb = model(r, jitter=torch.rand(RAYS, NC, device=dev), u=torch.rand(RAYS, NF, device=dev), **kw)[0]
            loss = torch.mean((rgb - gt) ** 2)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            if leg != "localise_frozen":
                model.update_coarse_sigma_grid()
        return step

    legs = {leg: make_leg(leg) for leg in ("train", "train_ray_grads", "localise_frozen")}
    for step in legs.values():
        step(); step()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.reps):
        for leg, step in legs.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            times[leg].append((time.perf_counter() - t0) / a.steps * 1e3)
    ms = {k: summary(v) for k, v in times.items()}
    doc = dict(tool="tools/bench_pose_refine.py", device=torch.cuda.get_device_name(0),
               config=f"BASELINE configs[3]: {RAYS} rays x ({NC} + {NF}), eager iterations", steps_per_leg=a.steps, reps=a.reps, ms_per_step=ms,
               ray_grads_cost_ms=ms["train_ray_grads"]["median"] - ms["train"]["median"])

    # (b) per call, one stream
    side = train.SIDE_STREAM_SCATTER
    train.SIDE_STREAM_SCATTER = False
    per_call = {}
    try:
        for _ in range(a.reps):
            train.KERNEL_MARKS = []
            train.mark("begin")
            legs["train_ray_grads"]()
            torch.cuda.synchronize()
            marks, seen = train.KERNEL_MARKS, {}
            for (_, e0), (name, e1) in zip(marks, marks[1:]):
                seen[name] = seen.get(name, 0) + 1
                key = name if name != "ego_march_density" else f"ego_march_density[{seen[name] - 1}]"
                per_call.setdefault(key, []).append(e0.elapsed_time(e1))
    finally:
        train.KERNEL_MARKS, train.SIDE_STREAM_SCATTER = None, side
    calls = {k: summary(v) for k, v in per_call.items()}
    med = lambda k: calls[k]["median"]
    doc["ms_per_call_one_stream"] = calls
    # [0] the coarse pass on the pooled tables, [1] the fine pass: the 18 density taps per sample ego_ray_grad re-reads
    gathers = med("ego_march_density[1]") + med("ego_shade")
    doc["ray_grad_vs_forward_gathers"] = dict(ego_ray_grad_ms=med("ego_ray_grad"), ego_view_grad_ms=med("ego_view_grad"),
                                              fine_march_plus_shade_ms=gathers, ratio=med("ego_ray_grad") / gathers)
    print(json.dumps(doc, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
