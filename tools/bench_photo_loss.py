"""The photometric term's cost on the device: the kernels next to torch's MSE and the depth kernel, and the captured training step.

    python tools/bench_photo_loss.py                                  # -> profiles/r24/photo_loss.json
    python tools/bench_photo_loss.py --only step --legs mse --package-root OTHER_TREE --key parent_step
                                                                      # the default-loss step, timed on another checkout's package

(a) kernel: `ego_photo_loss` (value + g_rgb [+ g_affine]: its three launches) at N = 8192 and 65536 - "plain" (no weight, image or affine,
    L2: the MSE), and "full" (weights with a masked tenth, image indices, an affine table, Charbonnier) for K = 16 / 100 / 1000 -
    `ego_photo_fit` at the same N and K, torch's `mean((rgb - target) ** 2)` forward + backward at the same N, and `ego_ray_depth_loss`
    at N x 256 for scale.  One process; per repetition every leg in turn, `calls` calls between two device events; the median over
    repetitions, with min and max as the spread.
(b) step: BASELINE configs[3] (8192 rays x (128 + 128)) as a replayed GraphedTrainStep whose batches are drawn inside the graph from a
    RayBank of 16 panoramas of 64 x 128 with masks: the default MSE lambda ("mse"), `photometric_loss(rgb, gt)` ("photo"), and
    `photometric_loss(rgb, gt, weight, image, ExposureDeltas(anchor=0).affine(), "charbonnier")` with the exposure parameters as an extra
    group of the step's FusedAdam ("full").  One model and optimiser per leg in one process, the legs alternated, `steps` replays
    between two device synchronisations; the median over repetitions.  On a checkout without the term (--package-root) only the "mse"
    leg exists.  Every run with the same --key is kept (a list), so that runs of two checkouts can be alternated by the caller and their
    spread seen.
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
SIZES = (8192, 65536)
KS = (16, 100, 1000)
DEPTH_S = 256
TRAIN_RAYS, TRAIN_NC, TRAIN_NF = 8192, 128, 128
BANK_K, BANK_H, BANK_W = 16, 64, 128


def summary(v) -> dict:
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), n=len(v))


def bench_kernels(reps: int, calls: int) -> dict:
    import torch
    from egonerf_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    st = _lib.stream_handle()
    legs = {}
    for N in SIZES:
        rgb = torch.rand(N, 3, device=dev, generator=g)
        target = (rgb + 0.05 * torch.randn(N, 3, device=dev, generator=g)).contiguous()
        weight = torch.rand(N, device=dev, generator=g)
        weight[::10] = 0.0
        g_rgb, value = torch.empty_like(rgb), torch.zeros(1, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.ego_photo_loss_workspace_bytes(N, max(KS)) // 8, dtype=torch.float64, device=dev)
        legs[f"photo_plain_{N}"] = ((rgb, target, g_rgb, value, ws), lambda c=rgb, t=target, gr=g_rgb, v=value, w=ws, N=N: _lib.check(
            lib.ego_photo_loss(c.data_ptr(), t.data_ptr(), None, None, None, N, 0, _lib.PHOTO_L2, 0.0, w.data_ptr(), v.data_ptr(), gr.data_ptr(),
                               None, st), "ego_photo_loss"))
        for K in KS:
            image = torch.randint(0, K, (N,), device=dev, generator=g, dtype=torch.int32)
            affine = torch.stack([0.7 + 0.6 * torch.rand(K, 3, device=dev, generator=g), 0.1 * torch.rand(K, 3, device=dev, generator=g) - 0.05], -1)
            affine = affine.contiguous()
            g_aff, fit = torch.empty_like(affine), torch.empty_like(affine)
            keep = (weight, image, affine, g_aff, fit)
            legs[f"photo_full_{N}_K{K}"] = (keep, lambda c=rgb, t=target, wt=weight, im=image, a=affine, gr=g_rgb, ga=g_aff, v=value, w=ws, N=N, K=K:
                                            _lib.check(lib.ego_photo_loss(c.data_ptr(), t.data_ptr(), wt.data_ptr(), im.data_ptr(), a.data_ptr(), N, K,
                                                                          _lib.PHOTO_CHARBONNIER, 1e-3, w.data_ptr(), v.data_ptr(), gr.data_ptr(),
                                                                          ga.data_ptr(), st), "ego_photo_loss"))
            legs[f"photo_fit_{N}_K{K}"] = (keep, lambda c=rgb, t=target, wt=weight, im=image, f=fit, N=N, K=K: _lib.check(
                lib.ego_photo_fit(c.data_ptr(), t.data_ptr(), wt.data_ptr(), im.data_ptr(), N, K, f.data_ptr(), None, st), "ego_photo_fit"))
        leaf = rgb.clone().requires_grad_(True)

        def torch_mse(c=leaf, t=target):
            c.grad = None
            torch.mean((c - t) ** 2).backward()
        legs[f"torch_mse_fwd_bwd_{N}"] = ((leaf,), torch_mse)
        alpha = (0.5 * torch.rand(N, DEPTH_S, device=dev, generator=g) ** 4).contiguous()
        z = (0.01 * 1500.0 ** torch.sort(torch.rand(N, DEPTH_S, device=dev, generator=g), dim=1).values).contiguous()
        dt = 0.01 + 15.0 * torch.rand(N, device=dev, generator=g)
        dt[::3] = 0.0
        g_alpha = torch.empty_like(alpha)
        dws = torch.empty(lib.ego_ray_depth_loss_workspace_bytes(N) // 8, dtype=torch.float64, device=dev)
        legs[f"depth_{N}x{DEPTH_S}"] = ((alpha, z, dt, g_alpha, dws), lambda a=alpha, z=z, t=dt, gr=g_alpha, v=value, w=dws, N=N: _lib.check(
            lib.ego_ray_depth_loss(a.data_ptr(), DEPTH_S, z.data_ptr(), t.data_ptr(), None, N, DEPTH_S, 0.01, 15.0, _lib.DIST_METRIC, _lib.DEPTH_L2,
                                   w.data_ptr(), v.data_ptr(), gr.data_ptr(), None, st), "ego_ray_depth_loss"))
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
    return dict(calls_per_leg=calls, reps=reps, plain="no weight / image / affine, l2, value + g_rgb (three launches)",
                full="weight (a tenth 0), image, affine, charbonnier, value + g_rgb + g_affine (three launches)",
                fit="weight, image: one launch", torch_mse="mean((rgb - target) ** 2) forward + backward, eager", us_per_call=us,
                full_minus_plain_us={f"{N}_K{K}": med(f"photo_full_{N}_K{K}") - med(f"photo_plain_{N}") for N in SIZES for K in KS},
                full_us_per_image={f"{N}": (med(f"photo_full_{N}_K{KS[-1]}") - med(f"photo_full_{N}_K{KS[0]}")) / (KS[-1] - KS[0]) for N in SIZES})


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
    masks = np.full((BANK_K, BANK_H, BANK_W), 255, np.uint8)
    masks[:, BANK_H * 7 // 8:] = 0   # the nadir
    has_masks = "masks" in inspect.signature(RayBank.__init__).parameters
    if not has_masks and set(legs) != {"mse"}:
        raise SystemExit("this checkout has no photometric term: only --legs mse can be timed on it")

    graphed = {}
    for leg in legs:
        model = synth.build_model(cfg, weights, dev)
        model.train()
        groups = model.get_optparam_groups(0.02, 1e-3)
        loss_fn = None   # "mse": the step's default lambda
        if leg == "photo":
            loss_fn = lambda rgb, tgt, alpha: losses.photometric_loss(rgb, tgt)
        elif leg == "full":
            from egonerf_amd.exposure import ExposureDeltas
            deltas = ExposureDeltas(BANK_K, device=dev, anchor=0)
            groups = groups + [dict(params=list(deltas.parameters()), lr=1e-3)]
            loss_fn = lambda rgb, tgt, alpha, weight, image, d=deltas: losses.photometric_loss(rgb, tgt, weight=weight, image=image,
                                                                                              affine=d.affine(), kind="charbonnier")
        opt = FusedAdam(groups, betas=(0.9, 0.99), capturable=True, lr_factor=0.1 ** (1 / 30000))
        bank = RayBank(poses, images, (BANK_W, BANK_H), device=dev, **(dict(masks=masks) if has_masks else {}))
        graphed[leg] = GraphedTrainStep(model, opt, render_kwargs=kw, loss_fn=loss_fn, warmup=2, batch_source=DeviceSimpleSampler(bank, TRAIN_RAYS, seed=3))
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
                      f"{BANK_K} x {BANK_H} x {BANK_W}" + (" with masks (the lowest eighth of every image)" if has_masks else ""),
               steps_per_leg=steps, reps=reps, ms_per_step=ms, final_loss={k: float(st.loss) for k, st in graphed.items()})
    if "mse" in ms:
        out["ms_over_mse"] = {k: ms[k]["median"] - ms["mse"]["median"] for k in ms if k != "mse"}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=["kernel", "step"], help="one of the two measurements (default: both)")
    ap.add_argument("--legs", nargs="+", default=["mse", "photo", "full"], choices=["mse", "photo", "full"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="kernel calls per leg and repetition")
    ap.add_argument("--steps", type=int, default=20, help="replays per leg and repetition")
    ap.add_argument("--package-root", default=HERE, help="the checkout whose egonerf_amd package is measured")
    ap.add_argument("--key", default="step", help="the key of --out whose list takes the step result")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r24", "photo_loss.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    if not torch.cuda.is_available():
        print("tools/bench_photo_loss.py needs a HIP device: a time from anything else says nothing", file=sys.stderr)
        return 1
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.update(tool="tools/bench_photo_loss.py", device=torch.cuda.get_device_name(0))
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
