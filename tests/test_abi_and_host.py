"""CPU-only checks: the C-ABI library loads and exports every declared symbol (no compute calls), host
logic (LUTs, schedules, resolution rule, samplers, parameter layout, sharding) and the failure mode
without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.coordinates import YinYangSphericalCoords
from egonerf_amd.renderer import psnr_from_sse, shard_bounds
from egonerf_amd.sampler import SimpleSampler, ThetaImportanceSampler
from tests.helpers import make_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    lib = _lib.load()
    names = _lib.header_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert set(names) == set(_lib.PROTOTYPES)  # the binding covers the whole header, nothing extra
    assert lib.ego_abi_version() == _lib.EXPECTED_ABI_VERSION == 17
    assert [lib.ego_sizeof(i) for i in range(3)] == [ctypes.sizeof(_lib.Scene), ctypes.sizeof(_lib.RenderArgs),
                                                     ctypes.sizeof(_lib.VmField)]
    assert lib.ego_packed_floats() == 2 * 46852 + 9216 + 2 * 36864  # fp32 layout + fp16-split layout + fp16-table basis fragments + f16f8 and f16f6 W1/W2


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    assert lib.ego_sample_ray_exp(None, None, None, 0.0, 4, 8, None, None, None) == -1
    assert b"sample_ray_exp" in lib.ego_last_error()
    sc = _lib.Scene()
    assert lib.ego_shade(sc, None, None, None, 1, 1, None, None, None, None) == -1
    assert lib.ego_render_workspace_bytes(4096, None) == -1
    a = _lib.RenderArgs()
    a.n_coarse, a.n_fine, a.resampling, a.use_coarse_sample = 128, 128, 1, 1
    need = lib.ego_render_workspace_bytes(4096, ctypes.byref(a))
    assert need >= 4 * 4096 * (128 * 2 + 256 * 2 + 1 + 256 * 3)


def test_train_layout_is_the_reference_input_order():
    """ego_train_layout(0) against a restatement of MLPRender_Fea's input (tensorBase.py:68-75, positional_encoding: feature-major
    over the frequencies, sines before cosines) mapped through the kernels' per-half slot rule; layouts 1-3 against the values
    recorded from the build before the layer-1 operand order got its single definition in ego_tuned.h."""
    lib = _lib.load()

    def layout(which, n):
        buf = (ctypes.c_int32 * n)()
        assert lib.ego_train_layout(which, buf, n) == 0
        return list(buf)

    D, PE = 27, 2  # app_dim, view_pe = fea_pe
    names = [("fea", f) for f in range(D)] + [("dir", d) for d in range(3)]
    names += [(fn, "fea", f, 2 ** j) for fn in ("sin", "cos") for f in range(D) for j in range(PE)]
    names += [(fn, "dir", d, 2 ** j) for fn in ("sin", "cos") for d in range(3) for j in range(PE)]
    assert len(names) == 150
    col = {nm: i for i, nm in enumerate(names)}
    # the 16 view slots over the two lane halves: the raw direction, then sin PE, then cos PE, then a pad
    view = [("dir", d) for d in range(3)] + [(fn, "dir", d, m) for fn in ("sin", "cos") for d in range(3) for m in (1, 2)] + [None]
    want = [None] * 160
    for h in range(2):
        for kk in range(80):
            if kk < 70:  # 14 feature slots x (f, sin f, sin 2f, cos f, cos 2f); register r of half h holds feature 2r + h
                f, kind = 2 * (kk // 5) + h, kk % 5
                nm = [("fea", f), ("sin", "fea", f, 1), ("sin", "fea", f, 2), ("cos", "fea", f, 1), ("cos", "fea", f, 2)][kind] if f < D else None
            else:
                nm = view[8 * h + kk - 70] if kk < 78 else None
            want[(kk >> 2) * 8 + h * 4 + (kk & 3)] = col[nm] if nm is not None else -1  # dump_col(kk, h)
    got = layout(0, 160)
    assert sorted(got) == [-1] * 10 + list(range(150))
    assert got == want

    assert layout(1, 128) == list(range(128))  # recorded: hidden unit = dump column
    assert layout(2, 32) == [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, -1, -1,
                             1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, -1, -1, -1]
    assert layout(3, 144) == [
        0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19, 20, 21, 22, 23, 32, 33, 34, 35, 36, 37, 38, 39,
        8, 9, 10, 11, 12, 13, 14, 15, 24, 25, 26, 27, 28, 29, 30, 31, 40, 41, 42, 43, 44, 45, 46, 47,
        48, 49, 50, 51, 52, 53, 54, 55, 64, 65, 66, 67, 68, 69, 70, 71, 80, 81, 82, 83, 84, 85, 86, 87,
        56, 57, 58, 59, 60, 61, 62, 63, 72, 73, 74, 75, 76, 77, 78, 79, 88, 89, 90, 91, 92, 93, 94, 95,
        96, 97, 98, 99, 100, 101, 102, 103, 112, 113, 114, 115, 116, 117, 118, 119, 128, 129, 130, 131, 132, 133, 134, 135,
        104, 105, 106, 107, 108, 109, 110, 111, 120, 121, 122, 123, 124, 125, 126, 127, 136, 137, 138, 139, 140, 141, 142, 143]


def test_resolution_rule_and_constants(golden):
    fx = golden("stages")
    cfg = synth.SceneConfig()
    c = YinYangSphericalCoords("cpu", cfg.aabb, exp_r=True, N_voxel=cfg.n_voxel, r0=cfg.r0, interval_th=True)
    assert c.resolution == [150, 172, 516]
    assert [c.N_to_reso(n ** 3) for n in (20, 40, 100)] == [[10, 10, 30], [20, 22, 64], [50, 56, 168]]
    assert float(c.far[0]) == float(fx["normr/full/far_r"])
    assert synth.n_to_reso(27e6) == c.resolution


def test_sample_schedules_bit_exact(golden):
    fx = golden("stages")
    for name, (near, far, r0) in dict(indoor=(0.01, 15.0, 0.03), ricoh=(0.1, 300.0, 0.05), mid=(0.01, 50.0, 0.05)).items():
        cfg = synth.SceneConfig(n_voxel=20 ** 3, near=near, far=far, r0=r0)
        c = YinYangSphericalCoords("cpu", cfg.aabb, exp_r=True, N_voxel=cfg.n_voxel, r0=r0, interval_th=True)
        for S in (32, 64, 128, 256, 512):
            z = near + c.sample_schedule(near, far, S)
            assert np.array_equal(z.numpy(), fx[f"sched/{name}/{S}"]), (name, S)


def test_r_lut_reproduces_reference_normalize_r(golden):
    """The host-built LUT + the searchsorted/lerp rule (restated in numpy) gives the reference's normalize_r."""
    fx = golden("stages")
    for name, nv in (("full", 27_000_000), ("tiny", 20 ** 3)):
        cfg = synth.SceneConfig(n_voxel=nv)
        c = YinYangSphericalCoords("cpu", cfg.aabb, exp_r=True, N_voxel=nv, r0=cfg.r0, interval_th=True)
        G = c.reference_r_grid().numpy()
        r = fx[f"normr/{name}/r"]
        k_out = np.clip(np.searchsorted(G, r, side="right"), 1, len(G) - 1)
        k_in = k_out - 1
        out = ((k_in.astype(np.float32) + (r - G[k_in]) / (G[k_out] - G[k_in])) / np.float32(c.N_r)).astype(np.float32)
        assert np.array_equal(out, fx[f"normr/{name}/out"])


def test_samplers_known_answers(golden):
    fx = golden("stages")
    np.random.seed(20221028)  # train.py:413
    s = SimpleSampler(10, 4)
    got = np.stack([s.nextids().numpy() for _ in range(5)])
    assert np.array_equal(got, fx["sampler/simple"])
    assert got.tolist()[0] == [5, 1, 0, 4]
    np.random.seed(20221028)
    t = ThetaImportanceSampler(5, 3, (8, 4), 6, [0, 1, 0, 1])
    assert np.allclose(t.weight, fx["sampler/theta_weight"], rtol=0, atol=1e-15)
    assert np.array_equal(np.asarray(t.nextids()), fx["sampler/theta_ids"])


def test_model_state_dict_matches_reference_manifest(golden):
    fx = golden("tiny")
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = synth.make_weights(cfg, seed=1234)
    model = make_model(cfg, w, "cpu")
    sd = model.state_dict()
    ref_keys = sorted(k[len("bw_grad/"):] for k in fx.files if k.startswith("bw_grad/"))  # the reference's named_parameters
    assert sorted(sd) == ref_keys and len(ref_keys) == 32
    for k in ref_keys:
        assert tuple(sd[k].shape) == fx["bw_grad/" + k].shape, k
        assert np.array_equal(sd[k].numpy(), w[k])
    p = model.density_plane_yin[0]
    assert p.shape == (1, 16, 10, 10) and p.permute(0, 2, 3, 1).is_contiguous()  # channel-last memory
    assert model.app_line_yang[2].permute(0, 2, 3, 1).is_contiguous()
    groups = model.get_optparam_groups(0.02, 1e-3, 0.005)
    assert len(groups) == 11 and [g["lr"] for g in groups[:5]] == [0.02] * 4 + [1e-3]


def test_no_cpu_fallback():
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    model = make_model(cfg, synth.make_weights(cfg, seed=1), "cpu")
    for call in (lambda: model(torch.zeros(4, 6), n_coarse=8, exp_sampling=True),
                 lambda: model.compute_densityfeature(torch.zeros(4, 7)),
                 lambda: model.compute_appfeature(torch.zeros(4, 7)),
                 lambda: model.coordinates.from_cartesian(torch.zeros(4, 3)),
                 lambda: model.feature2density(torch.zeros(4))):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_product_never_imports_the_oracle():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "egonerf_amd")
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f


def test_volume_renderer_passes_need_alpha_only_to_models_that_take_it():
    """keep_alpha=False drops the per-sample alpha; only this package's EgoNeRF (supports_need_alpha) is told not to produce it
    at all - a model with the reference's exact forward signature must keep working."""
    import torch
    from egonerf_amd.renderer import volume_renderer
    seen = []

    class RefLike:
        def __call__(self, rays_chunk, is_train=False, white_bg=True, ndc_ray=False, n_coarse=-1, n_fine=0, exp_sampling=False,
                     pivotal_sample_th=0.0, resampling=False, use_coarse_sample=True, interval_th=False, jitter=None, u=None):
            n = rays_chunk.shape[0]
            return torch.zeros(n, 3), torch.zeros(n), None, None, torch.ones(n, n_coarse)

    class Ours(RefLike):
        supports_need_alpha = True

        def __call__(self, rays_chunk, need_alpha=True, **kw):
            seen.append(need_alpha)
            out = RefLike.__call__(self, rays_chunk, **kw)
            return out if need_alpha else out[:4] + (None,)

    rays = torch.zeros(10, 6)
    for model in (RefLike(), Ours()):
        o = volume_renderer(rays, model, chunk=4, n_coarse=8, device="cpu", keep_alpha=False)
        assert o[0].shape == (10, 3) and o[4] is None
        o = volume_renderer(rays, model, chunk=4, n_coarse=8, device="cpu")
        assert o[4].shape == (10, 8)
    assert seen == [False] * 3 + [True] * 3


def test_shard_bounds_partition():
    for n, w in ((10, 3), (2048 * 1024, 8), (5, 8), (0, 2)):
        blocks = [shard_bounds(n, w, r) for r in range(w)]
        assert blocks[0][0] == 0 and blocks[-1][1] == n
        assert all(blocks[i][1] == blocks[i + 1][0] for i in range(w - 1))
        assert max(h - l for l, h in blocks) - min(h - l for l, h in blocks) <= 1
    assert abs(psnr_from_sse(0.01 * 300, 300) - 20.0) < 1e-12


def test_reference_checkpoint_loads_on_cpu(golden):
    """A `.th` file written by the reference's own EgoNeRF.save (tests/golden/reference_ckpt.th) unpickles through the
    module shims and rebuilds the model: kwargs objects, state_dict, packed alpha mask, envmap, global_step."""
    import sys
    from egonerf_amd.compat import load_reference_checkpoint
    from egonerf_amd.coordinates import YinYangSphericalCoords
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_ckpt.th")
    model, step = load_reference_checkpoint(path, device="cpu")
    assert step == 4321 and "models.coordinates" not in sys.modules  # shims are removed after the load
    cfg = synth.SceneConfig(n_voxel=20 ** 3, use_envmap=True, envmap_res_H=16)
    w = synth.make_weights(cfg, seed=77)
    for k, v in model.state_dict().items():
        assert np.array_equal(v.numpy(), w[k]), k
    assert isinstance(model.coordinates, YinYangSphericalCoords) and model.coordinates.resolution == [10, 10, 30]
    assert np.array_equal(model.coordinates.reference_r_grid().numpy(),
                          make_model(cfg, w, "cpu").coordinates.reference_r_grid().numpy())
    assert np.array_equal(model.envmap.emission.detach().numpy(), w["envmap.emission"])
    assert model.alphaMask is not None and tuple(model.alphaMask.alpha_volume_yin.shape) == (1, 1, 30, 10, 10)
    assert model.near_far == [0.01, 15.0] and model.density_shift == -8 and model.fea2denseAct == "softplus"


def _write_ckpt(tmp_path):
    cfg = synth.SceneConfig(n_voxel=20 ** 3, use_envmap=True, envmap_res_H=16)
    w = synth.make_weights(cfg, seed=77)
    model = make_model(cfg, w, "cpu")
    model.coordinates.lut_device("cpu")  # a populated LUT cache must not leak into the file
    path = str(tmp_path / "ours.th")
    model.save(path, 17)
    return cfg, w, model, path


def test_saved_checkpoint_uses_only_reference_class_paths(tmp_path):
    """EgoNeRF.save writes kwargs['coordinates'] / ['envmap'] as models.coordinates.YinYangSphericalCoords /
    models.envmap.EnvironmentMap with the reference's attribute sets (models/coordinates.py:75-82,206-215,500-505;
    models/envmap.py:17-24): the pickle names no egonerf_amd class and unpickles into bare stand-ins of those paths."""
    import copy, sys, types, zipfile
    cfg, w, model, path = _write_ckpt(tmp_path)
    with zipfile.ZipFile(path) as z:
        pkl = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    assert b"egonerf_amd" not in pkl and b"models.coordinates" in pkl and b"models.envmap" in pkl
    assert "models" not in sys.modules and "models.coordinates" not in sys.modules  # the save-time stand-ins are gone again
    pkg, mc, me = types.ModuleType("models"), types.ModuleType("models.coordinates"), types.ModuleType("models.envmap")
    pkg.__path__ = []
    mc.YinYangSphericalCoords = type("YinYangSphericalCoords", (), {"__module__": "models.coordinates"})
    me.EnvironmentMap = type("EnvironmentMap", (), {"__module__": "models.envmap"})
    sys.modules.update({"models": pkg, "models.coordinates": mc, "models.envmap": me})
    try:
        ck = torch.load(path, map_location="cpu", weights_only=False)
    finally:
        for n in ("models", "models.coordinates", "models.envmap"):
            sys.modules.pop(n, None)
    c, e = ck["kwargs"]["coordinates"], ck["kwargs"]["envmap"]
    assert type(c) is mc.YinYangSphericalCoords and type(e) is me.EnvironmentMap
    assert set(vars(c)) == {"center", "device", "near", "far", "inv_diff", "exp_r", "interval_th", "N_r", "N_theta", "N_phi", "r0", "ratio"}
    assert set(vars(e)) == {"emission"} and np.array_equal(e.emission.detach().numpy(), w["envmap.emission"])
    assert (c.N_r, c.N_theta, c.N_phi, c.r0, c.exp_r, c.interval_th) == (10, 10, 30, cfg.r0, True, True)
    assert torch.equal(c.far, model.coordinates.far) and c.ratio.dim() == 0
    assert set(ck) == {"kwargs", "state_dict", "global_step", "envmap.emission", "envmap_res_H"} and ck["global_step"] == 17
    # outside save(), ordinary pickling / deepcopy of the product's objects is untouched
    c2 = copy.deepcopy(model.coordinates)
    assert type(c2) is type(model.coordinates) and c2.resolution == [10, 10, 30]


def _load_with_stand_ins(path):
    """torch.load of a checkpoint whose pickle names the reference's class paths, into bare stand-ins of those paths."""
    import sys, types
    pkg, mc, me = types.ModuleType("models"), types.ModuleType("models.coordinates"), types.ModuleType("models.envmap")
    pkg.__path__ = []
    mc.YinYangSphericalCoords = type("YinYangSphericalCoords", (), {"__module__": "models.coordinates"})
    me.EnvironmentMap = type("EnvironmentMap", (), {"__module__": "models.envmap"})
    saved = {n: sys.modules.get(n) for n in ("models", "models.coordinates", "models.envmap")}
    sys.modules.update({"models": pkg, "models.coordinates": mc, "models.envmap": me})
    try:
        return torch.load(path, map_location="cpu", weights_only=False)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def _assert_same_content(a, b, where="ckpt"):
    """Same keys, types, values; tensors bit-equal with the same dtype and shape; objects compared attribute by attribute."""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b))
        for k in a:
            _assert_same_content(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same_content(x, y, f"{where}[{i}]")
    elif hasattr(a, "__dict__"):
        assert type(a).__module__ == type(b).__module__ and type(a).__name__ == type(b).__name__, where
        _assert_same_content(vars(a), vars(b), f"{where}.{type(a).__name__}")
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


def test_reference_opens_a_checkpoint_written_here(tmp_path, golden):
    """The real reference (fresh process, stub modules for its missing third-party imports) torch.loads a file written by
    EgoNeRF.save, rebuilds `EgoNeRF(**ckpt['kwargs'])`, `load(ckpt)`s it (train.py:52-56) and renders: oracle/capture_golden.py
    (capture_ours_checkpoint) recorded that file (tests/golden/ours_ckpt.th) and the reference's render of it.  The file written
    here today must carry exactly what the reference opened, and the reference's render must agree with the oracle."""
    from oracle.egonerf_oracle import OracleScene
    cfg, w, model, path = _write_ckpt(tmp_path)
    opened = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ours_ckpt.th")
    _assert_same_content(_load_with_stand_ins(path), _load_with_stand_ins(opened))
    out = golden("ours_ckpt_reference_render")
    rays = synth.make_rays(32, seed=5)
    assert np.array_equal(out["rays"], rays)
    assert int(out["step"]) == 17
    ref = OracleScene(cfg, w).forward(torch.from_numpy(rays), n_coarse=16, n_fine=16, resampling=True)
    assert np.abs(out["rgb"] - ref[0].numpy()).max() <= 2e-6 and np.abs(out["depth"] - ref[1].numpy()).max() <= 2e-5
    assert np.abs(out["env"] - ref[3].numpy()).max() <= 1e-6


def test_shipped_binary_has_no_high_half_broadcast_packed_fp32_ops():
    """every build of ego_shade.hip whose kernels contained packed fp32 instructions broadcasting the HIGH dword of
    a register pair (`v_pk_fma_f32 ... op_sel:[1,0,0]` without op_sel_hi) returned wrong results in some calls on MI355X; builds
    without them never did.  The check reads the code objects INSIDE the built libegonerf_hip.so (the binary that ships), not a
    fresh compile."""
    from egonerf_amd import build
    rep = build.shipped_isa_report()
    assert rep["code_objects"] >= 6
    assert rep["packed_fp32"] > 1000          # the check looked at real code
    assert not rep["high_half_broadcast"], rep["high_half_broadcast"][:5]


def build_faulty_variant(tmp_path):
    """The known-faulty form of the gather kernels (csrc/variants.h: -DEGO_PAIRED_WEIGHTS, SLP vectoriser on) as a side library."""
    import os
    from egonerf_amd import build
    out = str(tmp_path / "libegonerf_faulty.so")
    old = os.environ.get("EGO_NO_PER_FILE_FLAGS")
    os.environ["EGO_NO_PER_FILE_FLAGS"] = "1"
    try:
        build.build_library(force=True, extra=["-DEGO_PAIRED_WEIGHTS"], out=out)
    finally:
        if old is None:
            del os.environ["EGO_NO_PER_FILE_FLAGS"]
        else:
            os.environ["EGO_NO_PER_FILE_FLAGS"] = old
    return out


def test_isa_guard_sees_the_faulty_form(tmp_path):
    """The same check on a side build of the reproducer form finds the instructions, and that build's recorded hash can never pass
    for the product build's (an experiment build written over LIB used to keep the old .hash)."""
    from egonerf_amd import build
    out = build_faulty_variant(tmp_path)
    rep = build.shipped_isa_report(out)
    assert len(rep["high_half_broadcast"]) >= 12, rep
    assert open(out + ".hash").read().strip() != build.source_hash()
    assert open(build.LIB + ".hash").read().strip() == build.source_hash()


@pytest.mark.parametrize("flags", [["-DEGO_GATHER_TEAMS=0"], ["-DEGO_PAIRED_WEIGHTS"], ["-DEGO_WALK_PROF"]])
def test_kept_variants_compile(tmp_path, flags):
    """csrc/variants.h lists the compile-time variants kept on purpose (the section-5.1 reproducer forms); each must keep
    compiling for gfx950 next to the default build.  Everything else that was tried is recorded in DESIGN.md, not in #ifdefs."""
    import os, re, subprocess
    from egonerf_amd import build
    name = "ego_scatter_sorted.hip" if "WALK" in flags[0] else "ego_shade.hip"
    src = os.path.join(build.CSRC, name)
    macros = set(re.findall(r"\bEGO_[A-Z_]+\b", open(os.path.join(build.CSRC, "variants.h")).read()))
    assert flags[0][2:].split("=")[0] in macros
    cmd = [build._hipcc(), *build.COMMON_FLAGS, *build.EXTRA_FLAGS.get(name, []), *flags, "-c", src, "-o", str(tmp_path / "v.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # no other experiment switch hides in the kernel sources
    for f in sorted(os.listdir(build.CSRC)):
        text = open(os.path.join(build.CSRC, f)).read()
        stray = set(re.findall(r"#\s*if(?:n?def)?\s+(?:!?\s*defined\s*\(?\s*)?(EGO_[A-Z0-9_]+)", text)) - macros
        assert not stray, (f, stray)


def test_roctx_switch_loads_and_is_off_by_default():
    """EGO_ROCTX=1 (SURVEY 5 tracing row): the entry points open roctx ranges through a dlopen'ed roctx library - the library must load,
    the hooks must resolve (no stderr complaint) and a traced call must still return its normal status, with or without the switch."""
    import subprocess
    import sys
    code = ("from egonerf_amd import _lib; lib = _lib.load(); "
            "print(lib.ego_raw2alpha(None, None, 0, 4, None, None, None, None), lib.ego_sh_render(None, None, 5, None, None))")
    for switch in ("1", "0", None):
        env = {k: v for k, v in os.environ.items() if k != "EGO_ROCTX"}
        if switch is not None:
            env["EGO_ROCTX"] = switch
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == ["0", "-1"], r.stdout        # N = 0 is a no-op; a null argument is still refused inside a range
        assert "roctx" not in r.stderr, r.stderr


def test_sorted_scatter_argument_validation_needs_no_gpu():
    """ego_scatter_sorted_workspace_bytes / ego_scatter_sort refuse bad arguments before touching the device (csrc/ego_scatter_sort.hip, csrc/ego_sorted_geom.h)."""
    lib = _lib.load()
    sc = _lib.new_scene()
    assert lib.ego_scatter_sorted_workspace_bytes(None, 4, 4) == -1
    sc.density.res[:] = [150, 172, 516]
    sc.app.res[:] = [150, 172, 516]
    big = lib.ego_scatter_sorted_workspace_bytes(ctypes.byref(sc), 8192, 256)
    small = lib.ego_scatter_sorted_workspace_bytes(ctypes.byref(sc), 64, 32)
    assert big > small > 0 and big % 256 == 0
    assert lib.ego_scatter_sorted_workspace_bytes(ctypes.byref(sc), 1 << 24, 256) == -1     # N * S must stay below 2^31
    sc.density.res[:] = [150, 172, 5000]
    assert lib.ego_scatter_sorted_workspace_bytes(ctypes.byref(sc), 64, 32) == -1 and b"resolution" in lib.ego_last_error()
    sc.density.res[:] = [150, 172, 516]
    assert lib.ego_scatter_sort(ctypes.byref(sc), None, 4, 4, None, 0, None) == -1 and b"null" in lib.ego_last_error()
    assert lib.ego_scatter_sort(ctypes.byref(sc), None, 0, 4, None, 0, None) == 0                      # N = 0 is a no-op
    sc.app.res[:] = [150, 172, 500]
    assert lib.ego_scatter_sort(ctypes.byref(sc), 256, 4, 4, 256, 1 << 40, None) == -1 and b"one resolution" in lib.ego_last_error()
    assert lib.ego_weight_grad_partial_floats() == 1024 * 128 * 160


# ego_scatter_sorted_workspace_bytes of the library before the sort and the geometry left ego_scatter_sorted.hip, per grid for the
# batches (N, S) = (8192, 256), (48, 32), (1, 1): blocked and unblocked key layouts, dense and sparse cell buffers, a line that does not
# fit the walk ([8, 8, 4096]) and a grid whose blocked layout is refused ([8, 700, 3700])
_SORTED_WS_BATCHES = ((8192, 256), (48, 32), (1, 1))
_SORTED_WS_BYTES = {
    (150, 172, 516): (470647040, 47860224, 44220672),
    (300, 346, 1036): (3055684608, 92251904, 88612352),
    (10, 12, 34): (135331328, 21836800, 20269056),
    (2, 2, 2): (135277824, 16308992, 16239872),
    (8, 8, 4096): (184865536, 31831040, 28213504),
    (8, 8, 700): (136006400, 43047168, 39421952),
    (8, 700, 3700): (4996299264, 92387328, 88747776),
    (64, 64, 2000): (563446784, 58688000, 55048448),
}
# the same with EGO_SORTED_LINES=separate, and with EGO_SORTED_WALK=0 (no line blocks in the keys), for the first two batches
_SORTED_WS_BYTES_PLAIN = {
    (150, 172, 516): (387471104, 46606080),
    (10, 12, 34): (135331328, 21836800),
    (8, 700, 3700): (4996299264, 92387328),
}


def test_sorted_scatter_workspace_layout_is_pinned():
    """The workspace size is the end of the layout that the sort (csrc/ego_scatter_sort.hip) and the scatters (csrc/ego_scatter_sorted.hip)
    share through csrc/ego_sorted_geom.h: every sizing branch of make_geom must give the bytes it gave before the split."""
    lib = _lib.load()

    def table(grids, batches):
        out = {}
        for res in grids:
            sc = _lib.new_scene()
            sc.density.res[:] = list(res)
            sc.app.res[:] = list(res)
            out[res] = tuple(lib.ego_scatter_sorted_workspace_bytes(ctypes.byref(sc), n, s) for n, s in batches)
        return out

    switches = ("EGO_SORTED_LINES", "EGO_SORTED_WALK")
    saved = {k: os.environ.pop(k, None) for k in switches}
    try:
        assert table(_SORTED_WS_BYTES, _SORTED_WS_BATCHES) == _SORTED_WS_BYTES
        for key, value in (("EGO_SORTED_LINES", "separate"), ("EGO_SORTED_WALK", "0")):   # read per call
            os.environ[key] = value
            try:
                assert table(_SORTED_WS_BYTES_PLAIN, _SORTED_WS_BATCHES[:2]) == _SORTED_WS_BYTES_PLAIN, key
            finally:
                del os.environ[key]
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
