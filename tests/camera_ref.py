"""numpy restatements of csrc/ego_camera.hip's arithmetic, for tests/test_camera_host.py and tests/test_hip_camera_path.py.

`finish_ref` is renderer.py:227-233 and utils.py:14-25 as numpy evaluates them on float32 arrays - one rounding per operation - with
the one deliberate deviation of the kernel: an index outside [0, 256) saturates instead of wrapping."""
import numpy as np


def depth_range(near_far):
    """(mi, den) as numpy forms them from Python floats next to a float32 array: float32(mi), float32 of the double-precision sum."""
    mi, ma = float(near_far[0]), float(near_far[1])
    return np.float32(mi), np.float32(ma - mi + 1e-8)


def finish_ref(rgb, depth, near_far, palette=None):
    """-> (rgb8 [..., 3], idx8 [...], depth8 [..., 3] | None)."""
    rgb = np.asarray(rgb, np.float32)
    rgb8 = (np.clip(rgb, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)   # within [0, 255]: the cast is defined
    mi, den = depth_range(near_far)
    x = np.nan_to_num(np.asarray(depth, np.float32))
    with np.errstate(over="ignore"):
        v = np.float32(255) * ((x - mi) / den)
    assert v.dtype == np.float32
    idx8 = np.clip(v, np.float32(0), np.float32(255)).astype(np.uint8)   # saturation; truncation of [255, 256) is 255 as well
    return rgb8, idx8, (None if palette is None else np.asarray(palette, np.uint8).reshape(256, 3)[idx8])


def pinhole_dirs(H, W, focal, center, blender, index=None):
    """get_ray_directions / get_ray_directions_blender (dataLoader/ray_utils.py:43-82) in float32, operation by operation, for the
    row-major pixel indices `index` (default: all)."""
    index = np.arange(H * W) if index is None else np.asarray(index)
    col, row = (index % W).astype(np.float32), (index // W).astype(np.float32)
    cx, cy = (W / 2, H / 2) if center is None else center
    x = (col + np.float32(0.5) - np.float32(cx)) / np.float32(focal[0])
    y = (row + np.float32(0.5) - np.float32(cy)) / np.float32(focal[1])
    z = np.ones_like(x)
    return np.stack([x, -y, -z] if blender else [x, y, z], -1)
