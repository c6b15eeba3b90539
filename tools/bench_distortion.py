"""The distortion regulariser's cost on the device: the kernel next to the ray-entropy kernel, and the captured training step with it.

    python tools/bench_distortion.py                                  # -> profiles/r12/distortion.json
    python tools/bench_distortion.py --only step --legs mse entropy --package-root OTHER_TREE --key parent_step
                                                                      # the legs that exist there, timed on another checkout's package

(a) kernel: `ego_ray_distortion` ("log" space) and `ego_ray_entropy`, value and gradient, at 8192 x 256, 4096 x 512 and 8192 x 128, on
    alpha = 0.5 u^4 and an exponential z with sorted uniform exponents.  One process; per repetition every (kernel, shape) leg in turn,
    `calls` launches between two device events; the median over repetitions.  The ratios t(8192 x 256) / t(8192 x 128) and
    t(4096 x 512) / t(8192 x 256) say how the time scales: 2 and 1 for N S, 4 and 2 for N S^2.
(b) step: BASELINE configs[3] (8192 rays x (128 + 128), bench.py --config train) as a replayed GraphedTrainStep with the loss MSE,
    MSE + 1e-3 ray entropy, MSE + 1e-2 distortion: one model and optimiser per leg in one process, the legs alternated, `steps` replays
    between two device synchronisations; the median over repetitions.  The step gets faster as a fit proceeds; every leg has taken the
    same number of steps when it is timed.
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
SHAPES = ((8192, 256), (4096, 512), (8192, 128))
NEAR, FAR = 0.01, 15.0
TRAIN_RAYS, TRAIN_NC, TRAIN_NF = 8192, 128, 128


def summary(v) -> dict:
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), n=len(v))


def bench_kernels(reps: int, calls: int) -> dict:
    import torch
    from egonerf_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    legs = {}
    for N, S in SHAPES:
        alpha = (0.5 * torch.rand(N, S, device=dev, generator=g) ** 4).contiguous()
        z = (NEAR * (FAR / NEAR) ** torch.sort(torch.rand(N, S, device=dev, generator=g), dim=1).values).contiguous()
        grad, value = torch.empty_like(alpha), torch.zeros(1, dtype=torch.float64, device=dev)
        keep = (alpha, z, grad, value)
        st = _lib.stream_handle()
        legs[f"distortion_{N}x{S}"] = (keep, lambda a=alpha, z=z, gr=grad, v=value, N=N, S=S: _lib.check(
            lib.ego_ray_distortion(a.data_ptr(), S, z.data_ptr(), N, S, NEAR, FAR, _lib.DIST_LOG, v.data_ptr(), gr.data_ptr(), st), "ego_ray_distortion"))
        legs[f"entropy_{N}x{S}"] = (keep, lambda a=alpha, gr=grad, v=value, N=N, S=S: _lib.check(
            lib.ego_ray_entropy(a.data_ptr(), N, S, S, v.data_ptr(), gr.data_ptr(), st), "ego_ray_entropy"))
    for _, call in legs.values():   # warm-up: code objects
        call()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for name, (_, call) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls * 1e3)
    us = {k: summary(v) for k, v in times.items()}
    med = lambda k: us[k]["median"]
    return dict(calls_per_leg=calls, reps=reps, space="log", us_per_call=us,
                distortion_time_ratio={"8192x256 / 8192x128 (N S: 2, N S^2: 4)": med("distortion_8192x256") / med("distortion_8192x128"),
                                       "4096x512 / 8192x256 (N S: 1, N S^2: 2)": med("distortion_4096x512") / med("distortion_8192x256")},
                distortion_over_entropy={f"{N}x{S}": med(f"distortion_{N}x{S}") / med(f"entropy_{N}x{S}") for N, S in SHAPES})


def bench_step(legs, reps: int, steps: int) -> dict:
    import torch
    from egonerf_amd import losses, synth
    from egonerf_amd.optim import FusedAdam
    from egonerf_amd.train import GraphedTrainStep
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig()
    weights = synth.make_weights(cfg, seed=1234)
    rays = torch.from_numpy(synth.make_rays(TRAIN_RAYS, seed=1)).to(dev)
    gt = torch.from_numpy(synth.hash_uniform(3, 0, TRAIN_RAYS * 3).reshape(TRAIN_RAYS, 3).astype(np.float32)).to(dev)
    kw = dict(n_coarse=TRAIN_NC, n_fine=TRAIN_NF, exp_sampling=True, resampling=True, use_coarse_sample=True)
    mse = lambda rgb, tgt: torch.mean((rgb - tgt) ** 2)

    def loss_for(leg, model):
        if leg == "mse":
            return lambda rgb, tgt, alpha: mse(rgb, tgt)
        if leg == "entropy":
            return lambda rgb, tgt, alpha: mse(rgb, tgt) + 1e-3 * losses.ray_entropy_loss(alpha)
        return lambda rgb, tgt, alpha: mse(rgb, tgt) + 1e-2 * losses.distortion_loss(alpha, model.last_train_z, model.near_far)

    graphed = {}
    for leg in legs:
        model = synth.build_model(cfg, weights, dev)
        model.train()
        opt = FusedAdam(model.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=0.1 ** (1 / 30000))
        graphed[leg] = GraphedTrainStep(model, opt, rays, gt, kw, loss_fn=loss_for(leg, model), warmup=2)
    for st in graphed.values():
        st(rays, gt)
    torch.cuda.synchronize()
    times = {k: [] for k in graphed}
    for _ in range(reps):
        for leg, st in graphed.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                st(rays, gt)
            torch.cuda.synchronize()
            times[leg].append((time.perf_counter() - t0) / steps * 1e3)
    ms = {k: summary(v) for k, v in times.items()}
    out = dict(config="BASELINE configs[3]: 8192 rays x (128 + 128), GraphedTrainStep replays", steps_per_leg=steps, reps=reps, ms_per_step=ms,
               final_loss={k: float(st.loss) for k, st in graphed.items()})
    if "mse" in ms:
        out["ms_over_mse"] = {k: ms[k]["median"] - ms["mse"]["median"] for k in ms if k != "mse"}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=["kernel", "step"], help="one of the two measurements (default: both)")
    ap.add_argument("--legs", nargs="+", default=["mse", "entropy", "distortion"], choices=["mse", "entropy", "distortion"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="kernel launches per leg and repetition")
    ap.add_argument("--steps", type=int, default=20, help="replays per leg and repetition")
    ap.add_argument("--package-root", default=HERE, help="the checkout whose egonerf_amd package is measured")
    ap.add_argument("--key", help="--only step: the key of --out that takes the result (default: step)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r12", "distortion.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    if not torch.cuda.is_available():
        print("tools/bench_distortion.py needs a HIP device: a time from anything else says nothing", file=sys.stderr)
        return 1
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.update(tool="tools/bench_distortion.py", device=torch.cuda.get_device_name(0))
    if a.only != "step":
        doc["kernel"] = bench_kernels(a.reps, a.calls)
        print(json.dumps(doc["kernel"], indent=1), flush=True)
    if a.only != "kernel":
        key = a.key or "step"
        doc[key] = bench_step(a.legs, a.reps, a.steps)
        print(json.dumps(doc[key], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
