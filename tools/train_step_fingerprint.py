"""Fingerprint of the training step (egonerf_amd.train.RenderFunction): which library calls a step queues, and the bits it computes;
and of EgoNeRF.forward without a graph (inference_cases: the bits of every output, under no_grad).

    python tools/train_step_fingerprint.py OUT.json            one eager forward + backward per case (+ one GraphedTrainStep case),
                                                               one forward per inference case
    python tools/train_step_fingerprint.py --compare A.json B.json

Per case: the mark names collected through train.KERNEL_MARKS (one per library call, in queueing order) and the sha256 of the bytes of
rgb_map, depth, alpha and of every parameter gradient in named_parameters() order, from pinned rays / jitter / u / target
(egonerf_amd.synth).  Two checkouts that queue the same calls with the same arguments give the same file, except where float atomics
add in arrival order; those entries are listed under "excused" (derived from the case's own mark names: the atomic table scatters and
the environment map's gradient, csrc/ego_stages.hip::k_envmap_bwd; and every parameter gradient when model.deterministic_scatter is off,
which also turns ego_weight_grad's fixed-order sums into atomics).
--compare fails on any other difference.  Each case runs once; the first failure ends the run."""
import hashlib
import itertools
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from egonerf_amd import synth, train  # noqa: E402
from egonerf_amd.optim import FusedAdam  # noqa: E402

DEV = "cuda"
N = 333                      # with 24 samples per ray: N * S is not a multiple of the 32-sample tile
RESAMPLED = dict(n_coarse=16, n_fine=16, resampling=True, use_coarse_sample=True)
SINGLE = dict(n_coarse=24)
SWITCHES = ("SIDE_STREAM_SCATTER", "WALK_BASIS", "WALK_DV", "DUMP_X")
ATOMIC_MARKS = {"ego_scatter_density": "density_", "ego_scatter_generic(density)": "density_", "ego_scatter_app": "app_",
                "ego_scatter_generic(app)": "app_", "ego_envmap_backward": "envmap."}   # k_envmap_bwd: 12 float atomics per ray


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def uniform(stream: int, *shape) -> torch.Tensor:
    return torch.from_numpy(synth.hash_uniform(21, stream, int(np.prod(shape))).reshape(shape).astype(np.float32)).to(DEV)


def cases():
    """(name, SceneConfig keywords, model attributes, train switches, environment, render keywords, alpha loss)"""
    for rs, env, side in itertools.product((True, False), (False, True), (True, False)):
        yield (f"tuned resampling={int(rs)} envmap={int(env)} side_stream={int(side)}", dict(use_envmap=env, envmap_res_H=16), {},
               dict(SIDE_STREAM_SCATTER=side), {}, RESAMPLED if rs else SINGLE, False)
    yield "tuned DUMP_X", {}, {}, dict(DUMP_X=True), {}, RESAMPLED, False
    yield "tuned WALK_BASIS=False", {}, {}, dict(WALK_BASIS=False), {}, RESAMPLED, False
    yield "tuned WALK_DV=False", {}, {}, dict(WALK_DV=False), {}, RESAMPLED, False
    yield "tuned train_fp32_head", {}, dict(train_fp32_head=True), {}, {}, RESAMPLED, False
    yield "tuned deterministic_scatter=False", {}, dict(deterministic_scatter=False), {}, {}, RESAMPLED, False
    for mode, head in (("MLP", dict(shadingMode="MLP", app_dim=27, view_pe=2, fea_pe=2, featureC=128)), ("RGB", dict(shadingMode="RGB", app_dim=3))):
        for walk in ("1", "0"):
            yield f"{mode} head, 48-component tables, EGO_SORTED_WALK={walk}", head, {}, {}, dict(EGO_SORTED_WALK=walk), RESAMPLED, False
    yield "tuned head, 8-component density", dict(density_n_comp=(8, 8, 8)), {}, {}, {}, RESAMPLED, False
    yield "tuned, loss uses alpha", dict(use_envmap=True, envmap_res_H=16), {}, {}, {}, RESAMPLED, True


def inference_cases():
    """(name, SceneConfig keywords, model attributes, rays start outside the box, forward keywords).  Public names only: the same file
    runs against an older checkout.  The attribute "alpha_mask" stands for updateAlphaMask() + use_alpha_mask."""
    exp = dict(exp_sampling=True)
    yield "eval exp_sampling=1", {}, {}, False, dict(exp, **SINGLE)
    yield "eval exp_sampling=0, equal entry distances", {}, {}, False, dict(SINGLE)
    yield "eval exp_sampling=0, rays from outside the box (ray-0 distances)", {}, {}, True, dict(SINGLE)
    yield "eval exp_sampling=0, rays from outside the box, resampling", {}, {}, True, dict(RESAMPLED)
    yield "eval resampling", {}, {}, False, dict(exp, **RESAMPLED)
    yield "eval envmap", dict(use_envmap=True, envmap_res_H=16), {}, False, dict(exp, **RESAMPLED)
    yield ("eval alpha mask + weight threshold + early termination", {},
           dict(alpha_mask=True, use_weight_thres=True, rayMarch_weight_thres=2e-2, early_termination_eps=1e-3), False, dict(exp, **RESAMPLED))
    yield "eval app_table_dtype=f16", {}, dict(app_table_dtype="f16"), False, dict(exp, **RESAMPLED)
    for prec in ("f16f6", "f16f8", "f16x3", "f32"):
        yield f"eval mlp_precision={prec}", {}, dict(mlp_precision=prec), False, dict(exp, **RESAMPLED)
    yield "eval need_alpha=False", {}, {}, False, dict(exp, need_alpha=False, **RESAMPLED)


def run_inference_case(name, cfg_kw, attrs, outside, kw):
    attrs = dict(attrs)
    model = build(cfg_kw, {})
    model.eval()
    if attrs.pop("alpha_mask", False):
        model.updateAlphaMask()
        model.use_alpha_mask = True
    for k, v in attrs.items():
        setattr(model, k, v)
    rays = torch.from_numpy(synth.make_rays(N, seed=6)).to(DEV)
    if outside:   # every other ray starts well outside the aabb and looks back in: the entry distances differ from ray to ray
        far = 3.0 * float(model.aabb.abs().max())
        rays[1::2, :3] -= far * rays[1::2, 3:6]
    with torch.no_grad():
        out = model(rays, **kw)
        shaded = model.last_shaded_samples   # None: the call did not go through ego_render_forward
    torch.cuda.synchronize()
    assert (shaded is None) == outside, (name, "expected the ray-0-distance path" if outside else "expected ego_render_forward")
    hashes = {k: None if t is None else sha(t) for k, t in zip(("rgb_map", "depth", "bg_map", "env_map", "alpha"), out)}
    hashes["last_shaded_samples"] = None if shaded is None else int(shaded)
    return dict(marks=[], excused=[], sha256=hashes)


def build(cfg_kw, attrs):
    cfg = synth.SceneConfig(n_voxel=24 ** 3, **cfg_kw)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=5), DEV)
    model.train()
    for k, v in attrs.items():
        setattr(model, k, v)
    model.update_coarse_sigma_grid()
    return model


def named_grads(model):
    named = dict(model.named_parameters())
    if model.envmap is not None:
        named.setdefault("envmap.emission", model.envmap.emission)
    return named


def step(model, rays, target, kw, alpha_loss):
    jitter = uniform(1, N, kw["n_coarse"])
    u = uniform(2, N, kw["n_fine"]) if kw.get("resampling") else None
    rgb, depth, _bg, _env, alpha = model(rays, is_train=True, exp_sampling=True, jitter=jitter, u=u, **kw)
    loss = torch.mean((rgb - target) ** 2)
    if alpha_loss:
        loss = loss + 1e-2 * torch.mean(alpha * (1.0 - alpha))
    loss.backward()
    return rgb, depth, alpha


def run_case(name, cfg_kw, attrs, switches, env, kw, alpha_loss, timed_iterations=0):
    keep = {k: getattr(train, k) for k in SWITCHES}
    keep_env = {k: os.environ.get(k) for k in env}
    try:
        for k, v in switches.items():
            setattr(train, k, v)
        os.environ.update(env)
        model = build(cfg_kw, attrs)
        rays, target = torch.from_numpy(synth.make_rays(N, seed=6)).to(DEV), uniform(3, N, 3)
        train.KERNEL_MARKS = []
        rgb, depth, alpha = step(model, rays, target, kw, alpha_loss)
        torch.cuda.synchronize()
        marks, train.KERNEL_MARKS = [m for m, _ in train.KERNEL_MARKS], None
        out = dict(marks=marks, sha256=dict(rgb_map=sha(rgb), depth=sha(depth), alpha=sha(alpha)))
        grads = named_grads(model)
        for k, p in grads.items():
            out["sha256"]["grad/" + k] = None if p.grad is None else sha(p.grad)
        atomic = {ATOMIC_MARKS[m] for m in marks if m in ATOMIC_MARKS}
        out["excused"] = sorted("grad/" + k for k in grads if not model.deterministic_scatter or any(k.startswith(a) for a in atomic))
        if timed_iterations:   # for information: host-bound eager time of this small case
            for p in grads.values():
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(timed_iterations):
                step(model, rays, target, kw, alpha_loss)
            torch.cuda.synchronize()
            out["eager_ms_per_iteration"] = (time.perf_counter() - t0) / timed_iterations * 1e3
        return out
    finally:
        train.KERNEL_MARKS = None
        for k, v in keep.items():
            setattr(train, k, v)
        for k, v in keep_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def run_graphed():
    """GraphedTrainStep, default (sorted, bit-reproducible) step: 5 replays on changing batches, then every parameter hashed."""
    model = build({}, {})
    opt = FusedAdam(model.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=0.9)
    batches = [(torch.from_numpy(synth.make_rays(N, seed=40 + i)).to(DEV), uniform(10 + i, N, 3)) for i in range(5)]
    noise = {16: uniform(1, N, 16)}
    graphed = train.GraphedTrainStep(model, opt, batches[0][0], batches[0][1], dict(exp_sampling=True, **RESAMPLED), warmup=1,
                                     noise_fn=lambda n, m, dev: noise[m])
    for rays, target in batches:
        loss = graphed(rays, target)
    torch.cuda.synchronize()
    return dict(marks=[], excused=[], sha256=dict({"param/" + k: sha(p) for k, p in model.named_parameters()}, loss=sha(loss)))


def compare(a_path, b_path) -> int:
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = []
    if list(a["cases"]) != list(b["cases"]):
        bad.append("the case lists differ")
    for name in a["cases"]:
        ca, cb = a["cases"][name], b["cases"].get(name)
        if cb is None:
            continue
        if ca["marks"] != cb["marks"]:
            bad.append(f"{name}: mark lists differ\n  {ca['marks']}\n  {cb['marks']}")
        if ca["excused"] != cb["excused"] or list(ca["sha256"]) != list(cb["sha256"]):
            bad.append(f"{name}: entries / excused entries differ")
        bad += [f"{name}: {k} differs" for k, v in ca["sha256"].items() if k not in ca["excused"] and cb["sha256"].get(k) != v]
    n_hash = sum(len(c["sha256"]) - len(c["excused"]) for c in a["cases"].values())
    print("\n".join(bad) if bad else f"identical: {len(a['cases'])} cases, every mark list, {n_hash} hashes "
          f"({sum(len(c['excused']) for c in a['cases'].values())} float-atomic entries excused)")
    for k in ("eager_ms_per_iteration",):
        first = next(iter(a["cases"]))
        print(f"{k} of '{first}': {a['cases'][first].get(k)} vs {b['cases'].get(first, {}).get(k)}")
    return 1 if bad else 0


def main(argv):
    if argv[:1] == ["--compare"]:
        return compare(argv[1], argv[2])
    assert torch.cuda.is_available(), "needs a GPU"
    out = dict(device=torch.cuda.get_device_name(0), cases={})
    for i, case in enumerate(cases()):
        print("case:", case[0], flush=True)
        out["cases"][case[0]] = run_case(*case, timed_iterations=20 if i == 0 else 0)
    print("case: graphed step", flush=True)
    out["cases"]["GraphedTrainStep, 5 replays"] = run_graphed()
    for case in inference_cases():
        print("case:", case[0], flush=True)
        out["cases"][case[0]] = run_inference_case(*case)
    os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
    json.dump(out, open(argv[0], "w"), indent=1)
    print("wrote", argv[0])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
