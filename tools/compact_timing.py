"""Compact shading (ego_render_forward_compacts) against the tile path, alternated in one process: for the erp_masked scene (carved field,
reference alpha mask), the erp_opaque_field scene (density_shift 0, no mask) - both 1024 x 2048, 128 + 128 with resampling, 16384-ray
chunks - and the headline batch (4096 x 512), the live-sample fraction, the shaded-tile fraction, ms per chunk and s per image with
EGO_RENDER_COMPACT=0 and =1.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/compact_timing.py`.
Usage: python tools/compact_timing.py [--reps R] [--scenes erp_masked,erp_opaque_field,headline]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egonerf_amd import synth  # noqa: E402
from egonerf_amd.renderer import erp_rays, volume_renderer  # noqa: E402

DEV = torch.device("cuda", 0)
H, W, CHUNK = 1024, 2048, 16384
ERP_KW = dict(n_coarse=128, n_fine=128, exp_sampling=True, resampling=True, use_coarse_sample=True)


def set_compact(v):
    os.environ["EGO_RENDER_COMPACT"] = v


def scene(name):
    if name == "headline":
        cfg = synth.SceneConfig()
        model = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), DEV)
        return model, torch.from_numpy(synth.make_rays(4096, seed=1)).to(DEV), dict(n_coarse=512, exp_sampling=True), None
    cfg = synth.SceneConfig(**dict(synth.RICOH, **({"density_shift": 0.0} if name == "erp_opaque_field" else {})))
    w = synth.make_weights(cfg, seed=1234)
    if name == "erp_masked":
        w = synth.carve_empty_space(w, cfg)
    model = synth.build_model(cfg, w, DEV)
    if name == "erp_masked":
        with torch.no_grad():
            model.updateAlphaMask()
        model.use_alpha_mask = True
    pose = np.eye(4, dtype=np.float32)[:3]
    chunk = erp_rays(H, W, pose, DEV, H // 3, -(-CHUNK // W))[:CHUNK].contiguous()   # a chunk from the image's middle third
    return model, chunk, ERP_KW, pose


def ms_per_call(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="alternations of the two paths")
    ap.add_argument("--scenes", default="erp_masked,erp_opaque_field,headline")
    a = ap.parse_args()
    out = {}
    for name in a.scenes.split(","):
        model, rays, kw, pose = scene(name)
        N = rays.shape[0]
        S = kw["n_coarse"] + kw.get("n_fine", 0)
        res = dict(default_compacts=None, live_fraction=None, shaded_tile_fraction=None, ms_per_chunk={"0": [], "1": []},
                   s_per_image={"0": [], "1": []})
        with torch.no_grad():
            os.environ.pop("EGO_RENDER_COMPACT", None)
            from egonerf_amd import _lib
            res["default_compacts"] = int(_lib.load().ego_render_forward_compacts(model.scene(), N, S))
            for v in ("1", "0"):
                set_compact(v)
                model(rays, **kw)
                n = int(model.last_shaded_samples)
                res["live_fraction" if v == "1" else "shaded_tile_fraction"] = n / (N * S)
            image_rays = erp_rays(H, W, pose, DEV) if pose is not None else None
            for _ in range(a.reps):
                for v in ("0", "1"):
                    set_compact(v)
                    res["ms_per_chunk"][v].append(round(ms_per_call(lambda: model(rays, **kw), 20), 4))
                    if image_rays is not None:
                        res["s_per_image"][v].append(round(ms_per_call(lambda: volume_renderer(image_rays, model, chunk=CHUNK, device=DEV,
                                                                                                 keep_alpha=False, **kw), 2) / 1e3, 4))
        os.environ.pop("EGO_RENDER_COMPACT", None)
        for k in ("ms_per_chunk", "s_per_image"):
            res[k + "_median"] = {v: (float(np.median(x)) if x else None) for v, x in res[k].items()}
        out[name] = res
        print(name, json.dumps(res), flush=True)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
