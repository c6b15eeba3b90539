"""How much slower are the any-shape compatibility kernels (csrc/ego_generic.hip) than the tuned path?  ("about an order
of magnitude" deserves a number.)  Same grid, same rays: the shipped shape against shapes that take the compatibility kernels for the head
(shadingMode 'MLP', featureC 64, view_pe = fea_pe = 6) - inference at 4096 x 512 and one training step at 8192 x (128 + 128).
`march`: only the any-shape density march (k_march_generic, 8 density components) at 4096 x 512 and 16384 x 128, event-timed per launch
like tools/march_timing.py, with checksums.  `--lib PATH`: time another build of the library (one process per build)."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egonerf_amd import _lib, synth
if "--lib" in sys.argv:
    i = sys.argv.index("--lib")
    os.environ["EGO_ALLOW_STALE_LIB"] = "1"   # the timed build is not the tree's
    _lib.LIB = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
dev = "cuda"
if "march" in sys.argv[1:]:
    cfg = synth.SceneConfig(density_n_comp=(8, 8, 8), app_n_comp=(24, 24, 24), featureC=64)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), dev)
    lib, st, sc = _lib.load(), _lib.stream_handle(), model.scene()
    def run(N, S, reps=100):
        rays, sched = torch.from_numpy(synth.make_rays(N, seed=1)).to(dev), model._sched(S, dev)
        z, w, bg, crd = torch.empty(N, S, device=dev), torch.empty(N, S, device=dev), torch.empty(N, device=dev), torch.empty(N, S, 4, device=dev)
        act = torch.empty(N * S // 32 + 1, device=dev, dtype=torch.uint8)
        go = lambda: _lib.check(lib.ego_march_density(sc, rays.data_ptr(), N, S, None, sched.data_ptr(), None, cfg.near, 0, z.data_ptr(), None, 0, w.data_ptr(),
                                                      bg.data_ptr(), crd.data_ptr(), None, act.data_ptr(), st), "march")
        t_end = time.perf_counter() + 0.2
        while time.perf_counter() < t_end:
            for _ in range(8): go()
            torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        for i in range(reps):
            ev[i].record(); go()
        ev[reps].record(); torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)])), float(w.double().sum()), float(crd.double().abs().sum())
    a, b = run(4096, 512), run(16384, 128)
    print(f"generic march 4096x512 {a[0]*1e3:.1f} us | 16384x128 {b[0]*1e3:.1f} us | checksums {a[1]:.6f} {a[2]:.3f} {b[1]:.6f} {b[2]:.3f}")
    sys.exit(0)
SHAPES = {"shipped (MFMA path)": {}, "shadingMode MLP (generic head)": dict(shadingMode="MLP"), "featureC 64, small tables (generic)": dict(density_n_comp=(8, 8, 8), app_n_comp=(24, 24, 24), featureC=64),
          "ctor defaults 6 / 6 encodings (generic)": dict(view_pe=6, fea_pe=6, app_dim=12)}
def ms(fn, reps):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps
for name, kw in SHAPES.items():
    cfg = synth.SceneConfig(**kw)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), dev)
    rays = torch.from_numpy(synth.make_rays(4096, seed=1)).to(dev)
    with torch.no_grad():
        t_inf = ms(lambda: model(rays, n_coarse=512, exp_sampling=True), 10)
    model.train()
    rays8 = torch.from_numpy(synth.make_rays(8192, seed=1)).to(dev); gt = torch.rand(8192, 3, device=dev)
    def step():
        model.zero_grad(set_to_none=True)
        rgb, *_ = model(rays8, is_train=True, n_coarse=128, n_fine=128, exp_sampling=True, resampling=True, use_coarse_sample=True)
        torch.mean((rgb - gt) ** 2).backward()
    t_tr = ms(step, 3)
    print(f"{name:42s} tuned={model.is_tuned_shape!s:5s} inference 4096 x 512: {t_inf:8.3f} ms   training fwd+bwd 8192 x (128+128): {t_tr:8.2f} ms", flush=True)
