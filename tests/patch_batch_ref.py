"""Numpy restatement of the patch mode of the device batch generator (csrc/ego_batch.hip: k_ray_batch_sample_patches; the rule is stated at
ego_ray_batch_sample_patches in include/egonerf_hip.h), on the Philox of tests/ray_bank_ref.py.  Shared by tests/test_patch_ssim_host.py
(properties of the rule, no GPU) and tests/test_hip_patch_ssim.py (the device's indices against it, as arrays)."""
import numpy as np

from tests.ray_bank_ref import U32, philox4x32_10

PATCH_KEY_TWEAK, RANDOM_KEY_TWEAK = 0x50415443, 0x52414E44


def _hi(x, n):
    return ((x * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def wraps(c0, n_cols, W):
    return c0 == 0 and n_cols == W


def patch_origins(K, n_rows, n_cols, wrap, patches, patch, stride, seed, counter):
    """-> (img, row0, col0) of the iteration's patches, int64 [patches]"""
    ph, pw = patch
    p = np.arange(patches, dtype=np.uint64)
    x = philox4x32_10((p & U32, p >> np.uint64(32), counter & 0xFFFFFFFF, counter >> 32),
                      ((seed & 0xFFFFFFFF) ^ PATCH_KEY_TWEAK, seed >> 32))
    col_origins = n_cols if wrap else n_cols - (pw - 1) * stride
    return _hi(x[0], K), _hi(x[1], n_rows - (ph - 1) * stride), _hi(x[2], col_origins)


def random_pixels(K, n_rows, n_cols, n_random, seed, counter):
    """-> (img, row, col) of the iteration's trailing independent pixels, int64 [n_random]"""
    r = np.arange(n_random, dtype=np.uint64)
    x = philox4x32_10((r & U32, r >> np.uint64(32), counter & 0xFFFFFFFF, counter >> 32),
                      ((seed & 0xFFFFFFFF) ^ RANDOM_KEY_TWEAK, seed >> 32))
    return _hi(x[0], K), _hi(x[2], n_rows), _hi(x[1], n_cols)


def patch_pixels(n_cols, wrap, row0, col0, patch, stride):
    """-> (rows [P, ph], cols [P, pw]) of patches with given origins"""
    ph, pw = patch
    rows = row0[:, None] + np.arange(ph) * stride
    cols = col0[:, None] + np.arange(pw) * stride
    return rows, (cols % n_cols if wrap else cols)


def patch_batch_indices(K, n_rows, n_cols, wrap, patches, patch, stride, n_random, seed, counter):
    """The indices of iteration `counter`, int64 [patches * ph * pw + n_random], in the bank's index space."""
    img, row0, col0 = patch_origins(K, n_rows, n_cols, wrap, patches, patch, stride, seed, counter)
    rows, cols = patch_pixels(n_cols, wrap, row0, col0, patch, stride)
    idx = img[:, None, None] * (n_rows * n_cols) + rows[:, :, None] * n_cols + cols[:, None, :]
    ri, rr, rc = random_pixels(K, n_rows, n_cols, n_random, seed, counter)
    return np.concatenate([idx.reshape(-1), ri * (n_rows * n_cols) + rr * n_cols + rc])
