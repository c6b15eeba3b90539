"""CPU-only checks of the device-resident training batches (include/egonerf_hip.h: ego_ray_bank, ego_ray_batch_gather,
ego_ray_batch_sample; egonerf_amd.data.RayBank; egonerf_amd.sampler.Device*Sampler): exports and argument validation without a GPU,
the host state of the bank and of the samplers, and the properties of the generator the kernels implement, on its numpy restatement
(tests/ray_bank_ref.py; tests/test_hip_ray_bank.py holds the device to that restatement bit for bit)."""
import ctypes

import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from egonerf_amd.data import RayBank
from egonerf_amd.sampler import DeviceSimpleSampler, DeviceThetaImportanceSampler, ThetaImportanceSampler
from tests import ray_bank_ref as ref


def _struct(**kw):
    b = _lib.RayBankStruct(poses=64, images=64, K=2, H=4, W=8, r0=0, n_rows=4, c0=0, n_cols=8, normalize=1)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name in ("ego_ray_batch_gather", "ego_ray_batch_sample"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and name in _lib.header_symbols()
    assert lib.ego_abi_version() == 17          # append-only additions
    assert lib.ego_sizeof(5) == ctypes.sizeof(_lib.RayBankStruct) == 48
    assert lib.ego_sizeof(6) == -1


def test_gather_argument_validation_needs_no_gpu():
    lib = _lib.load()
    call = lambda b, idx=64, B=4, rays=64, rgb=64: lib.ego_ray_batch_gather(ctypes.byref(b) if b is not None else None, idx, B, rays, rgb, None)
    bad = [(None, {}), (_struct(poses=None), {}), (_struct(images=None), {}), (_struct(K=0), {}), (_struct(r0=1), {}), (_struct(n_rows=0), {}),
           (_struct(c0=4, n_cols=5), {}), (_struct(c0=-1), {}), (_struct(), dict(B=-1)), (_struct(), dict(idx=None)),
           (_struct(), dict(rays=None, rgb=None))]
    for b, kw in bad:
        assert call(b, **kw) == -1, kw
        assert b"ray_batch_gather" in lib.ego_last_error(), lib.ego_last_error()
    assert call(_struct(), B=0) == 0                                  # B == 0 is a no-op
    assert call(_struct(images=None), B=0, rgb=None) == 0             # a bank without images serves rays


def test_sample_argument_validation_needs_no_gpu():
    lib = _lib.load()

    def call(b, mode=0, counter=64, cdf=None, B=4, idx=64, rays=64, rgb=64):
        return lib.ego_ray_batch_sample(ctypes.byref(b) if b is not None else None, mode, 7, counter, cdf, B, idx, rays, rgb, None)

    bad = [(None, {}), (_struct(poses=None), {}), (_struct(images=None), {}), (_struct(K=0), {}), (_struct(r0=2, n_rows=3), {}),
           (_struct(), dict(B=-1)), (_struct(), dict(mode=2)), (_struct(), dict(mode=-1)),
           (_struct(), dict(mode=1, cdf=None)),                        # theta_importance without its table
           (_struct(), dict(mode=0, B=33)),                            # simple: 64 rays do not hold two batches of 33
           (_struct(), dict(counter=None)), (_struct(), dict(idx=None))]
    for b, kw in bad:
        assert call(b, **kw) == -1, kw
        assert b"ray_batch_sample" in lib.ego_last_error(), lib.ego_last_error()
    assert b"idx" in lib.ego_last_error()
    assert call(_struct(), B=0) == 0
    assert call(_struct(), mode=1, cdf=64, B=0) == 0


def _host_bank(K=3, H=8, W=16, roi=(0, 1, 0, 1), channels=4):
    g = np.random.default_rng(3)
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    return RayBank(poses, g.integers(0, 256, (K, H, W, channels), dtype=np.uint8), (W, H), roi=roi, device="cpu")


def test_bank_host_state_and_no_cpu_fallback():
    b = _host_bank(roi=(0.25, 1.0, 0.0, 0.5))
    assert (b.r0, b.n_rows, b.c0, b.n_cols) == (2, 6, 0, 8) and b.total == len(b) == 3 * 6 * 8
    assert b.nbytes == 3 * 8 * 16 * 4 + 3 * 48
    assert (b.struct.K, b.struct.H, b.struct.W, b.struct.r0, b.struct.n_rows, b.struct.c0, b.struct.n_cols, b.struct.normalize) == (3, 8, 16, 2, 6, 0, 8, 1)
    rgb = _host_bank(channels=3)
    assert rgb.images.shape == (3, 8, 16, 4) and bool((rgb.images[..., 3] == 255).all()) and rgb.nbytes == b.nbytes
    with pytest.raises(RuntimeError, match="HIP device"):
        b.gather(torch.arange(4))
    with pytest.raises(RuntimeError, match="HIP device"):
        DeviceSimpleSampler(b, 8, seed=1).next_batch()
    with pytest.raises(ValueError):
        RayBank(np.zeros((2, 4, 4)), np.zeros((3, 8, 16, 4), np.uint8), (16, 8), device="cpu")
    with pytest.raises(ValueError):
        RayBank(np.zeros((3, 4, 4)), np.zeros((3, 8, 16, 4), np.float32), (16, 8), device="cpu")
    with pytest.raises(ValueError, match="two batches"):
        DeviceSimpleSampler(b, b.total // 2 + 1)


@pytest.mark.parametrize("roi", [(0, 1, 0, 1), (0.25, 1.0, 0.0, 0.5)])
def test_theta_cdf_is_the_host_samplers_cumulative_weight(roi):
    b = _host_bank(K=2, H=40, W=16, roi=roi)
    s = DeviceThetaImportanceSampler(5.0, b, 32, seed=9)
    host = ThetaImportanceSampler(5.0, 2, (16, 40), 32, list(roi))
    want = np.cumsum(host.weight).astype(np.float32)
    want[-1] = 1.0
    assert s.cdf_host.dtype == np.float32 and np.array_equal(s.cdf_host, want) and np.array_equal(s.cdf.numpy(), want)
    assert len(want) == b.n_rows and np.all(np.diff(want) > 0)
    assert s.counter.dtype == torch.int64 and int(s.counter) == 0
    s.seek(11)
    assert int(s.counter) == 11


def test_philox_known_answers():
    """Random123's published vectors for philox4x32-10 (kat_vectors: zero, all ones, the digits of pi)."""
    h = lambda c: [int(x) for x in c]
    assert h(ref.philox4x32_10((0, 0, 0, 0), (0, 0))) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert h(ref.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF))) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert h(ref.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


@pytest.mark.parametrize("total", [10007, 4096, 64, 2, 5, 1 << 15])
def test_feistel_map_is_a_bijection_per_epoch(total):
    """A prime, powers of two (even and odd bit counts), the fixture's own 64 and the smallest domains."""
    pos = np.arange(total)
    perms = [ref.feistel_permute(pos, total, seed=0x1234ABCD5678, epoch=e) for e in (0, 1, 2, 1 << 33)]
    for p in perms:
        assert p.min() == 0 and p.max() == total - 1 and np.array_equal(np.sort(p), pos)
    if total > 5:
        for i in range(len(perms)):
            for j in range(i):
                assert not np.array_equal(perms[i], perms[j])          # another epoch, another permutation
        assert not np.array_equal(perms[0], pos)
        assert not np.array_equal(perms[0], ref.feistel_permute(pos, total, seed=0x1234ABCD5679, epoch=0))   # ... another seed too
    assert 4 ** ref.half_bits(total) >= total and (ref.half_bits(total) == 1 or 4 ** (ref.half_bits(total) - 1) < total)


def test_simple_rule_follows_the_reference_epochs():
    """sampler.py:11-16: floor(total / batch) batches per permutation, the tail dropped; here for total 64 and 10 007."""
    for total, batch in ((64, 12), (10007, 1000)):
        per_epoch = total // batch
        seen = np.concatenate([ref.simple_indices(total, batch, 5, c) for c in range(per_epoch)])
        assert len(np.unique(seen)) == per_epoch * batch and seen.max() < total and seen.min() >= 0
        nxt = ref.simple_indices(total, batch, 5, per_epoch)
        assert not np.array_equal(nxt, seen[:batch])
        whole = ref.feistel_permute(np.arange(total), total, 5, 0)
        assert np.array_equal(seen, whole[:per_epoch * batch])
        assert np.array_equal(nxt, ref.feistel_permute(np.arange(batch), total, 5, 1))
