"""Numpy restatement of the device batch generator (csrc/ego_batch.hip): Philox4x32-10, the Feistel bijection with cycle-walking and
the two sampling rules of ego_ray_batch_sample.  Test infrastructure shared by tests/test_ray_bank_host.py (properties of the map, no
GPU) and tests/test_hip_ray_bank.py (the device's indices against it, bit for bit)."""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32-valued arrays (held as uint64), key: (k0, k1) ints -> four arrays."""
    c = [np.asarray(x, dtype=np.uint64) & U32 for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & U32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def feistel_f(r, key):
    x = (r + np.uint64(key)) & U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & U32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & U32
    x ^= x >> np.uint64(16)
    return x


def half_bits(total):
    half = 1
    while half < 31 and (1 << (2 * half)) < total:
        half += 1
    return half


def round_keys(seed, epoch):
    keys = []
    for j in range(2):
        keys += [int(x) for x in philox4x32_10((epoch & 0xFFFFFFFF, epoch >> 32, j, 0x46656973), (seed & 0xFFFFFFFF, seed >> 32))]
    return keys[:6]


def feistel_permute(p, total, seed, epoch):
    """positions p (array, all < total) -> their images under the epoch's bijection of [0, total)."""
    half, keys = np.uint64(half_bits(total)), round_keys(seed, epoch)
    mask = (np.uint64(1) << half) - np.uint64(1)
    v = np.asarray(p, dtype=np.uint64).copy()
    todo = np.ones(v.shape, dtype=bool)
    while todo.any():
        w = v[todo]
        L, R = (w >> half) & mask, w & mask
        for k in keys:
            L, R = R, L ^ (feistel_f(R, k) & mask)
        v[todo] = (L << half) | R
        todo = v >= np.uint64(total)
    return v.astype(np.int64)


def simple_indices(total, batch, seed, counter):
    per_epoch = total // batch
    epoch, in_epoch = counter // per_epoch, counter % per_epoch
    return feistel_permute(in_epoch * batch + np.arange(batch), total, seed, epoch)


def theta_draws(K, n_cols, cdf, batch, seed, counter):
    """-> (img, col, row) of the theta_importance rule; cdf = the float32 table."""
    lane = np.arange(batch, dtype=np.uint64)
    x = philox4x32_10((lane & U32, lane >> np.uint64(32), counter & 0xFFFFFFFF, counter >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    img = (x[0] * np.uint64(K)) >> np.uint64(32)
    col = (x[1] * np.uint64(n_cols)) >> np.uint64(32)
    u = (x[2] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    row = np.minimum(np.searchsorted(np.asarray(cdf, dtype=np.float32), u, side="right"), len(cdf) - 1)
    return img.astype(np.int64), col.astype(np.int64), row.astype(np.int64)


def theta_indices(K, n_rows, n_cols, cdf, batch, seed, counter):
    img, col, row = theta_draws(K, n_cols, cdf, batch, seed, counter)
    return img * (n_rows * n_cols) + row * n_cols + col
