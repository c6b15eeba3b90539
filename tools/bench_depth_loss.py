"""The depth term's cost on the device: the kernel next to the distortion kernel, and the captured training step with it.

    python tools/bench_depth_loss.py                                  # -> profiles/r22/depth_loss.json
    python tools/bench_depth_loss.py --only step --legs mse --package-root OTHER_TREE --key parent_step
                                                                      # the MSE-only step, timed on another checkout's package

(a) kernel: `ego_ray_depth_loss` ("metric", "l2", with a tail; value and gradient: its three launches) and `ego_ray_distortion` ("log"),
    at 8192 x 256, 4096 x 512 and 8192 x 128, on alpha = 0.5 u^4, an exponential z with sorted uniform exponents and targets in
    [near, far] of which a third are 0.  One process; per repetition every (kernel, shape) leg in turn, `calls` calls between two device
    events; the median over repetitions, with min and max as the spread.
(b) step: BASELINE configs[3] (8192 rays x (128 + 128)) as a replayed GraphedTrainStep whose batches are drawn inside the graph from a
    RayBank of 4 panoramas of 64 x 128 with depths, with the loss MSE and MSE + stepped(0.1, 0.5, 5000) * depth_loss: one model and
    optimiser per leg in one process, the legs alternated, `steps` replays between two device synchronisations; the median over
    repetitions.  On a checkout without depth support (--package-root) the bank has no depths and only the MSE leg exists.  Every run
    with the same --key is kept (a list), so that runs of two checkouts can be alternated by the caller and their spread seen.
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
BANK_K, BANK_H, BANK_W = 4, 64, 128


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
        target = NEAR + (FAR - NEAR) * torch.rand(N, device=dev, generator=g)
        target[::3] = 0.0
        tail = torch.rand(N, device=dev, generator=g)
        grad, value = torch.empty_like(alpha), torch.zeros(1, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.ego_ray_depth_loss_workspace_bytes(N) // 8, dtype=torch.float64, device=dev)
        keep = (alpha, z, target, tail, grad, value, ws)
        st = _lib.stream_handle()
        legs[f"depth_{N}x{S}"] = (keep, lambda a=alpha, z=z, t=target, tl=tail, gr=grad, v=value, w=ws, N=N, S=S: _lib.check(
            lib.ego_ray_depth_loss(a.data_ptr(), S, z.data_ptr(), t.data_ptr(), tl.data_ptr(), N, S, NEAR, FAR, _lib.DIST_METRIC, _lib.DEPTH_L2,
                                   w.data_ptr(), v.data_ptr(), gr.data_ptr(), None, st), "ego_ray_depth_loss"))
        legs[f"distortion_{N}x{S}"] = (keep, lambda a=alpha, z=z, gr=grad, v=value, N=N, S=S: _lib.check(
            lib.ego_ray_distortion(a.data_ptr(), S, z.data_ptr(), N, S, NEAR, FAR, _lib.DIST_LOG, v.data_ptr(), gr.data_ptr(), st), "ego_ray_distortion"))
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
    return dict(calls_per_leg=calls, reps=reps, depth="metric, l2, tail, value + gradient (three launches)", distortion="log, value + gradient",
                us_per_call=us, depth_over_distortion={f"{N}x{S}": med(f"depth_{N}x{S}") / med(f"distortion_{N}x{S}") for N, S in SHAPES})


def bench_step(legs, reps: int, steps: int) -> dict:
    import inspect
    import torch
    from egonerf_amd import losses, synth
    from egonerf_amd.data import RayBank
    from egonerf_amd.optim import FusedAdam
    from egonerf_amd.sampler import DeviceSimpleSampler
    from egonerf_amd.train import GraphedTrainStep
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig()
    weights = synth.make_weights(cfg, seed=1234)
    kw = dict(n_coarse=TRAIN_NC, n_fine=TRAIN_NF, exp_sampling=True, resampling=True, use_coarse_sample=True)
    g = np.random.default_rng(5)
    q, _ = np.linalg.qr(g.standard_normal((BANK_K, 3, 3)))
    poses = np.tile(np.eye(4, dtype=np.float32), (BANK_K, 1, 1))
    poses[:, :3, :3] = q
    poses[:, :3, 3] = g.uniform(-0.25, 0.25, (BANK_K, 3))
    images = g.integers(0, 256, (BANK_K, BANK_H, BANK_W, 4), dtype=np.uint8)
    depths = g.uniform(0.5, 6.0, (BANK_K, BANK_H, BANK_W)).astype(np.float32)
    depths[g.uniform(size=depths.shape) < 0.3] = 0
    has_depth = "depths" in inspect.signature(RayBank.__init__).parameters
    if not has_depth and "depth" in legs:
        raise SystemExit("this checkout's RayBank takes no depths: only --legs mse can be timed on it")
    mse = lambda rgb, tgt: torch.mean((rgb - tgt) ** 2)

    def loss_for(leg, model):
        if leg == "mse":
            return lambda rgb, tgt, alpha: mse(rgb, tgt)
        return lambda rgb, tgt, alpha, sched, depth: mse(rgb, tgt) + sched.stepped(0.1, 0.5, 5000) * losses.depth_loss(alpha, model.last_train_z, depth)

    graphed = {}
    for leg in legs:
        model = synth.build_model(cfg, weights, dev)
        model.train()
        opt = FusedAdam(model.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=0.1 ** (1 / 30000))
        bank = RayBank(poses, images, (BANK_W, BANK_H), device=dev, **(dict(depths=depths) if has_depth else {}))
        graphed[leg] = GraphedTrainStep(model, opt, render_kwargs=kw, loss_fn=loss_for(leg, model), warmup=2,
                                        batch_source=DeviceSimpleSampler(bank, TRAIN_RAYS, seed=3))
    for st in graphed.values():
        st()
    torch.cuda.synchronize()
    times = {k: [] for k in graphed}
    for _ in range(reps):
        for leg, st in graphed.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                st()
            torch.cuda.synchronize()
            times[leg].append((time.perf_counter() - t0) / steps * 1e3)
    ms = {k: summary(v) for k, v in times.items()}
    out = dict(config=f"BASELINE configs[3]: 8192 rays x (128 + 128), GraphedTrainStep replays, batches drawn in the graph from a bank of "
                      f"{BANK_K} x {BANK_H} x {BANK_W}" + (" with depths" if has_depth else " (no depth support in this checkout)"),
               steps_per_leg=steps, reps=reps, ms_per_step=ms, final_loss={k: float(st.loss) for k, st in graphed.items()})
    if "mse" in ms:
        out["ms_over_mse"] = {k: ms[k]["median"] - ms["mse"]["median"] for k in ms if k != "mse"}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=["kernel", "step"], help="one of the two measurements (default: both)")
    ap.add_argument("--legs", nargs="+", default=["mse", "depth"], choices=["mse", "depth"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="kernel calls per leg and repetition")
    ap.add_argument("--steps", type=int, default=20, help="replays per leg and repetition")
    ap.add_argument("--package-root", default=HERE, help="the checkout whose egonerf_amd package is measured")
    ap.add_argument("--key", default="step", help="the key of --out whose list takes the step result")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r22", "depth_loss.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    if not torch.cuda.is_available():
        print("tools/bench_depth_loss.py needs a HIP device: a time from anything else says nothing", file=sys.stderr)
        return 1
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.update(tool="tools/bench_depth_loss.py", device=torch.cuda.get_device_name(0))
    if a.only != "step":
        doc["kernel"] = bench_kernels(a.reps, a.calls)
        print(json.dumps(doc["kernel"], indent=1), flush=True)
    if a.only != "kernel":
        doc.setdefault(a.key, []).append(bench_step(a.legs, a.reps, a.steps))
        print(json.dumps(doc[a.key][-1], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
