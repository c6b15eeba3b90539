"""The structural term's and the patch sampler's cost on the device: the kernels next to torch, and the captured training step.

    python tools/bench_patch_ssim.py                                  # -> profiles/r25/patch_ssim.json
    python tools/bench_patch_ssim.py --only step --legs simple_mse --package-root OTHER_TREE --key parent_step
                                                                      # the default step, timed on another checkout's package

(a) kernel: `ego_patch_ssim` (value + g_rgb: its three launches) at 128 / 1024 patches of 8 x 8 (filter 7) and 32 / 256 patches of 16 x 16
    (filter 11), next to a torch eager SSIM - the five window moments by grouped `conv2d` with the same taps in float64, forward plus
    backward - on the same tensors.  One process; per repetition every leg in turn, `calls` calls between two device events; the median
    over repetitions, with min and max as the spread.
(b) sampler: one `sample_into` launch (indices, rays and colours) of DevicePatchSampler (96 patches of 8 x 8 plus 2048 random rows = 8192)
    and of DeviceSimpleSampler at 8192, timed the same way.
(c) step: BASELINE configs[3] (8192 rays x (128 + 128)) as a replayed GraphedTrainStep whose batches are drawn inside the graph from a
    RayBank of 16 panoramas of 64 x 128: DeviceSimpleSampler with the default MSE ("simple_mse": what the parent commit runs),
    DevicePatchSampler (96 patches of 8 x 8 plus 2048 random) with the default MSE ("patch_mse") and with 0.8 MSE + 0.2
    `patch_ssim_loss` ("patch_ssim").  One model and optimiser per leg in one process, the legs alternated, `steps` replays between two
    device synchronisations; the median over repetitions.  On a checkout without patch batches (--package-root) only "simple_mse" exists.
    Every run with the same --key is kept (a list), so that runs of two checkouts can be alternated by the caller and their spread seen.
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
KERNEL_CASES = ((128, 8, 7), (1024, 8, 7), (32, 16, 11), (256, 16, 11))   # patches, side, filter
TRAIN_RAYS, TRAIN_NC, TRAIN_NF = 8192, 128, 128
PATCHES, SIDE, N_RANDOM, LAM = 96, 8, 2048, 0.2
BANK_K, BANK_H, BANK_W = 16, 64, 128
LEGS = ("simple_mse", "patch_mse", "patch_ssim")


def summary(v) -> dict:
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), n=len(v))


def timed(legs: dict, reps: int, calls: int) -> dict:
    """us per call of every leg: per repetition every leg in turn, `calls` calls between two device events"""
    import torch
    for call in legs.values():   # warm-up: code objects
        call()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for name, call in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls * 1e3)
    return {k: summary(v) for k, v in times.items()}


def torch_ssim_loss(x, y, P, side, fs, taps):
    """1 - mean SSIM of [P * side * side, 3] patch rows by grouped conv2d in float64 (the definition, without the metric's guards)"""
    import torch
    import torch.nn.functional as F
    xi = x.double().view(P, side, side, 3).permute(0, 3, 1, 2)
    yi = y.double().view(P, side, side, 3).permute(0, 3, 1, 2)
    k = (taps[:, None] * taps[None, :]).expand(15, 1, fs, fs)
    m = F.conv2d(torch.cat([xi, yi, xi * xi, yi * yi, xi * yi], 1), k, groups=15)
    mux, muy, exx, eyy, exy = m.split(3, 1)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    sxx, syy, sxy = exx - mux * mux, eyy - muy * muy, exy - mux * muy
    return 1.0 - (((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sxx + syy + C2))).mean()


def bench_kernels(reps: int, calls: int) -> dict:
    import torch
    from egonerf_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    st = _lib.stream_handle()
    legs, keep, check = {}, [], {}
    for P, side, fs in KERNEL_CASES:
        n = P * side * side
        target = torch.rand(n, 3, device=dev, generator=g)
        rgb = (target + 0.05 * torch.randn(n, 3, device=dev, generator=g)).clamp(0, 1).contiguous()
        g_rgb, value = torch.empty_like(rgb), torch.zeros(1, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.ego_patch_ssim_workspace_bytes(P, side, side) // 8, dtype=torch.float64, device=dev)
        hw = fs // 2
        f = torch.exp(-0.5 * ((torch.arange(fs, dtype=torch.float64, device=dev) - hw + (2 * hw - fs + 1) / 2) / 1.5) ** 2)
        taps = f / f.sum()
        leaf = rgb.clone().requires_grad_(True)
        keep.append((target, rgb, g_rgb, value, ws, taps, leaf))
        tag = f"{P}x{side}x{side}_fs{fs}"
        legs[f"patch_ssim_{tag}"] = lambda c=rgb, t=target, gr=g_rgb, v=value, w=ws, P=P, s=side, fs=fs: _lib.check(
            lib.ego_patch_ssim(c.data_ptr(), t.data_ptr(), None, P, s, s, fs, 1.5, 1.0, 0.01, 0.03, w.data_ptr(), v.data_ptr(), gr.data_ptr(), st),
            "ego_patch_ssim")

        def torch_leg(c=leaf, t=target, P=P, s=side, fs=fs, k=taps):
            c.grad = None
            torch_ssim_loss(c, t, P, s, fs, k).backward()
        legs[f"torch_ssim_fwd_bwd_{tag}"] = torch_leg
        legs[f"patch_ssim_{tag}"]()
        torch_leg()
        check[tag] = dict(value=float(value), torch_value=float(torch_ssim_loss(rgb, target, P, side, fs, taps)),
                          g_max_abs_diff=float((g_rgb - leaf.grad).abs().max()), g_max_abs=float(leaf.grad.abs().max()))
    us = timed(legs, reps, calls)
    return dict(calls_per_leg=calls, reps=reps, patch_ssim="no weight, value + g_rgb (three launches)",
                torch_ssim="five window moments by grouped conv2d in float64, forward + backward, eager", us_per_call=us, agreement=check,
                torch_over_kernel={t: us[f"torch_ssim_fwd_bwd_{t}"]["median"] / us[f"patch_ssim_{t}"]["median"] for t in check})


def make_bank(dev):
    from egonerf_amd.data import RayBank
    g = np.random.default_rng(5)
    q, _ = np.linalg.qr(g.standard_normal((BANK_K, 3, 3)))
    poses = np.tile(np.eye(4, dtype=np.float32), (BANK_K, 1, 1))
    poses[:, :3, :3] = q
    poses[:, :3, 3] = g.uniform(-0.25, 0.25, (BANK_K, 3))
    images = g.integers(0, 256, (BANK_K, BANK_H, BANK_W, 4), dtype=np.uint8)
    return RayBank(poses, images, (BANK_W, BANK_H), device=dev)


def bench_sampler(reps: int, calls: int) -> dict:
    import torch
    from egonerf_amd.sampler import DevicePatchSampler, DeviceSimpleSampler
    dev = torch.device("cuda", 0)
    bank = make_bank(dev)
    idx = torch.empty(TRAIN_RAYS, dtype=torch.int64, device=dev)
    rays, rgb = torch.empty(TRAIN_RAYS, 6, device=dev), torch.empty(TRAIN_RAYS, 3, device=dev)
    simple = DeviceSimpleSampler(bank, TRAIN_RAYS, seed=3)
    patch = DevicePatchSampler(bank, patches=PATCHES, patch=(SIDE, SIDE), n_random=N_RANDOM, seed=3)
    us = timed(dict(simple=lambda: simple.sample_into(idx, rays, rgb), patch=lambda: patch.sample_into(idx, rays, rgb)), reps, calls)
    return dict(calls_per_leg=calls, reps=reps, batch=TRAIN_RAYS, patch=f"{PATCHES} patches of {SIDE} x {SIDE} + {N_RANDOM} random",
                what="one sample_into launch: indices, rays and colours", us_per_call=us)


def bench_step(legs, reps: int, steps: int) -> dict:
    import torch
    from egonerf_amd import sampler, synth
    from egonerf_amd.optim import FusedAdam
    from egonerf_amd.train import GraphedTrainStep
    dev = torch.device("cuda", 0)
    if not hasattr(sampler, "DevicePatchSampler") and set(legs) != {"simple_mse"}:
        raise SystemExit("this checkout has no patch batches: only --legs simple_mse can be timed on it")
    cfg = synth.SceneConfig()
    weights = synth.make_weights(cfg, seed=1234)
    kw = dict(n_coarse=TRAIN_NC, n_fine=TRAIN_NF, exp_sampling=True, resampling=True, use_coarse_sample=True)
    graphed = {}
    for leg in legs:
        model = synth.build_model(cfg, weights, dev)
        model.train()
        opt = FusedAdam(model.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=0.1 ** (1 / 30000))
        bank = make_bank(dev)
        loss_fn = None   # the step's default lambda: the MSE
        if leg == "simple_mse":
            src = sampler.DeviceSimpleSampler(bank, TRAIN_RAYS, seed=3)
        else:
            src = sampler.DevicePatchSampler(bank, patches=PATCHES, patch=(SIDE, SIDE), n_random=N_RANDOM, seed=3)
            if leg == "patch_ssim":
                from egonerf_amd.losses import patch_ssim_loss
                loss_fn = lambda rgb, tgt, alpha: (1 - LAM) * torch.mean((rgb - tgt) ** 2) + LAM * patch_ssim_loss(rgb, tgt, (SIDE, SIDE),
                                                                                                                   n_patches=PATCHES)
        graphed[leg] = GraphedTrainStep(model, opt, render_kwargs=kw, loss_fn=loss_fn, warmup=2, batch_source=src)
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
                      f"{BANK_K} x {BANK_H} x {BANK_W}; patch legs: {PATCHES} patches of {SIDE} x {SIDE} + {N_RANDOM} random, lambda {LAM}",
               steps_per_leg=steps, reps=reps, ms_per_step=ms, final_loss={k: float(st.loss) for k, st in graphed.items()})
    if "simple_mse" in ms:
        out["ms_over_simple_mse"] = {k: ms[k]["median"] - ms["simple_mse"]["median"] for k in ms if k != "simple_mse"}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=["kernel", "sampler", "step"], help="one of the three measurements (default: all)")
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=LEGS)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="kernel calls per leg and repetition")
    ap.add_argument("--steps", type=int, default=20, help="replays per leg and repetition")
    ap.add_argument("--package-root", default=HERE, help="the checkout whose egonerf_amd package is measured")
    ap.add_argument("--key", default="step", help="the key of --out whose list takes the step result")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r25", "patch_ssim.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    if not torch.cuda.is_available():
        print("tools/bench_patch_ssim.py needs a HIP device: a time from anything else says nothing", file=sys.stderr)
        return 1
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.update(tool="tools/bench_patch_ssim.py", device=torch.cuda.get_device_name(0))
    if a.only in (None, "kernel"):
        doc["kernel"] = bench_kernels(a.reps, a.calls)
        print(json.dumps(doc["kernel"], indent=1), flush=True)
    if a.only in (None, "sampler"):
        doc["sampler"] = bench_sampler(a.reps, a.calls)
        print(json.dumps(doc["sampler"], indent=1), flush=True)
    if a.only in (None, "step"):
        doc.setdefault(a.key, []).append(bench_step(a.legs, a.reps, a.steps))
        print(json.dumps(doc[a.key][-1], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
