"""Host side of egonerf_amd.model that needs no device: the sampling-noise plan of EgoNeRF.forward, the table storage functions of
egonerf_amd.field_tables, and the key of the scene cache.  Everything runs on a CPU-resident model."""
import itertools

import pytest
import torch

from egonerf_amd import field_tables, synth
from tests.helpers import make_model

N, N_COARSE, N_FINE = 5, 8, 4


def _cpu_model(interval_th=True):
    cfg = synth.SceneConfig(n_voxel=10 ** 3, interval_th=interval_th)
    return make_model(cfg, synth.make_weights(cfg, seed=11), "cpu")


@pytest.fixture(scope="module")
def models():
    return {th: _cpu_model(th) for th in (True, False)}


@pytest.fixture(scope="module")
def rays():
    return torch.from_numpy(synth.make_rays(N, seed=4))[:, :6].contiguous().float()


def _plan(model, rays, is_train, exp_sampling, resampling, jitter=None, u=None):
    return model._noise_plan(rays, N_COARSE, N_FINE, is_train, exp_sampling, resampling, jitter, u)


MODES = list(itertools.product((False, True), (False, True), (False, True)))   # exp_sampling, interval_th, resampling


@pytest.mark.parametrize("exp_sampling,interval_th,resampling", MODES)
def test_noise_plan_draws_in_the_documented_order(models, rays, exp_sampling, interval_th, resampling):
    """Training, nothing pinned.  The draws, in order: jitter [N, n_coarse] (CPU generator); where that jitter goes into explicit
    distances (the uniform schedule, the plain exponential schedule) a second [N, n_coarse] draw whose values the march never reads
    and which is what the call hands on as `jitter`; with resampling u [N, n_fine] from the generator of the rays' device (for CPU
    rays the same generator, so a draw out of order changes every later value)."""
    model = models[interval_th]
    torch.manual_seed(123)
    z, jitter, u = _plan(model, rays, True, exp_sampling, resampling)
    after = torch.rand(1)
    torch.manual_seed(123)
    first = torch.rand(N, N_COARSE)
    if not exp_sampling:
        want_z, want_jitter = model.sample_ray_z(rays, N_COARSE, first), torch.rand(N, N_COARSE)
    elif not interval_th:
        want_z, want_jitter = model._plain_exp_train_z(N_COARSE, first), torch.rand(N, N_COARSE)
    else:
        want_z, want_jitter = None, first
    want_u = torch.rand(N, N_FINE) if resampling else None
    want_after = torch.rand(1)
    assert (z is None) == (want_z is None) and (z is None or torch.equal(z, want_z))
    assert jitter.shape == (N, N_COARSE) and jitter.dtype == torch.float32 and torch.equal(jitter, want_jitter)
    assert (u is None) == (want_u is None) and (u is None or torch.equal(u, want_u))
    assert torch.equal(after, want_after)   # pins the discarded draw: one more or one fewer moves the generator


@pytest.mark.parametrize("exp_sampling,interval_th,resampling", MODES)
def test_noise_plan_draws_nothing_when_the_noise_is_pinned(models, rays, exp_sampling, interval_th, resampling):
    model = models[interval_th]
    g = torch.Generator().manual_seed(9)
    pin_j, pin_u = torch.rand(N, N_COARSE, generator=g), torch.rand(N, N_FINE, generator=g)
    state = torch.get_rng_state()
    z, jitter, u = _plan(model, rays, True, exp_sampling, resampling, pin_j, pin_u)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(jitter, pin_j) and ((u is None) if not resampling else torch.equal(u, pin_u))
    if not exp_sampling:
        assert torch.equal(z, model.sample_ray_z(rays, N_COARSE, pin_j))
    elif not interval_th:
        assert torch.equal(z, model._plain_exp_train_z(N_COARSE, pin_j))
    else:
        assert z is None


@pytest.mark.parametrize("exp_sampling,interval_th,resampling", MODES)
def test_noise_plan_of_an_eval_call_has_no_noise(models, rays, exp_sampling, interval_th, resampling):
    model = models[interval_th]
    state = torch.get_rng_state()
    for pinned in ((None, None), (torch.zeros(N, N_COARSE), torch.zeros(N, N_FINE))):
        z, jitter, u = _plan(model, rays, False, exp_sampling, resampling, *pinned)
        assert jitter is None and u is None
        assert (z is None) if exp_sampling else torch.equal(z, model.sample_ray_z(rays, N_COARSE))
    assert torch.equal(torch.get_rng_state(), state)


# ---- field_tables -------------------------------------------------------------------------------------------------------------------
def test_tables_returns_the_canonical_order():
    model = _cpu_model()
    for kind in ("density", "app"):
        want = [getattr(model, f"{kind}_{what}_{g}")[i] for g in ("yin", "yang") for what in ("plane", "line") for i in range(3)]
        got = field_tables.tables(model, kind)
        assert len(got) == 12 and all(a is b for a, b in zip(got, want))
    model.coarse_sigma_plane_yin[1] = marker = torch.zeros(1, 1, 1, 1)
    assert field_tables.tables(model, "density", coarse=True)[1] is marker


def _extent(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_carved_tables_are_channel_last_aligned_disjoint_and_compact(dtype):
    shapes = [(3, 5, 7), (4, 9, 1), (1, 1, 1), (16, 11, 13)]   # sizes that are no multiple of the 256-byte alignment
    views = field_tables.carve_channel_last(shapes, "cpu", dtype)
    base = views[0].untyped_storage().data_ptr()   # the allocator's alignment (256 bytes or more on the device, 64 for host memory)
    for v, (C_, H, W) in zip(views, shapes):
        assert v.shape == (1, C_, H, W) and v.dtype == dtype
        assert v.permute(0, 2, 3, 1).is_contiguous() and (v.data_ptr() - base) % 256 == 0
    spans = sorted(_extent(v) for v in views)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert field_tables.is_compact(views)
    assert len({v.untyped_storage().data_ptr() for v in views}) == 1


def test_recarve_in_place_keeps_parameter_objects_and_values():
    model = _cpu_model()
    for p in field_tables.tables(model, "app"):   # separate allocations, as after Module._apply or load_state_dict(assign=True)
        p.data = p.data.clone(memory_format=torch.preserve_format)
    ids = [id(p) for p in model.parameters()]
    want = [p.detach().clone() for p in field_tables.tables(model, "app")]
    assert len({p.untyped_storage().data_ptr() for p in field_tables.tables(model, "app")}) == 12
    field_tables.recarve(model, "app", keep_parameters=True)
    got = field_tables.tables(model, "app")
    assert [id(p) for p in model.parameters()] == ids
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert len({p.untyped_storage().data_ptr() for p in got}) == 1 and field_tables.is_compact(got)
    assert all(p.permute(0, 2, 3, 1).is_contiguous() for p in got)


def test_recarve_with_new_parameters_keeps_values_and_requires_grad():
    model = _cpu_model()
    olds = field_tables.tables(model, "density")
    olds[2].requires_grad_(False)
    olds[7].requires_grad_(False)
    want, names = [p.detach().clone() for p in olds], [n for n, _p in model.named_parameters()]
    field_tables.recarve(model, "density", keep_parameters=False)
    got = field_tables.tables(model, "density")
    assert all(isinstance(p, torch.nn.Parameter) for p in got) and not {id(p) for p in got} & {id(p) for p in olds}
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert [p.requires_grad for p in got] == [k not in (2, 7) for k in range(12)]
    assert len({p.untyped_storage().data_ptr() for p in got}) == 1
    assert [n for n, _p in model.named_parameters()] == names and not {id(p) for p in model.parameters()} & {id(p) for p in olds}


# ---- the scene key ------------------------------------------------------------------------------------------------------------------
def test_scene_key_follows_everything_the_struct_depends_on():
    model = _cpu_model()
    keys = [model._scene_key(False)]
    assert model._scene_key(False) == keys[0]   # nothing changed: same key

    def changed(what):
        key = model._scene_key(False)
        assert key not in keys, what
        assert model._scene_key(False) == key, what
        keys.append(key)

    model.use_alpha_mask = True; changed("use_alpha_mask")
    model.early_termination_eps = 1e-3; changed("early_termination_eps")
    model.use_weight_thres = True; changed("use_weight_thres")
    model.rayMarch_weight_thres = 2.5e-4; changed("rayMarch_weight_thres")
    model.skip_zero_weight_tiles = not model.skip_zero_weight_tiles; changed("skip_zero_weight_tiles")
    model.mlp_precision = "f16x3"; changed("mlp_precision")
    model.app_table_dtype = "f16"; changed("app_table_dtype")
    with torch.no_grad():
        model.renderModule.mlp[2].weight.mul_(1.0)
    changed("in-place write to an MLP weight")
    with torch.no_grad():
        model.app_line_yang[1].mul_(1.0)
    changed("in-place write to an appearance table while the half copy is in use")
    assert model._scene_key(True) not in keys and model._scene_key(True) == model._scene_key(True)
