"""What a mesh extraction costs on the device: the field on a lattice, the count and the emit of the extractor, and the
point gradients at the vertices, per stage, next to ego_march_density on the same scene in the same run.

    python tools/bench_mesh.py            # -> profiles/r19/mesh.json

Two lattices on the headline scene (synth.SceneConfig(), bench.py's): a 256^3 box of half the far distance around the centre and a
(128, 512, 1024) panorama lattice with geometric radii from the near to the far distance.  The level is the 0.9 quantile of the lattice's
own values, so a tenth of the nodes are inside.  Per lattice the four legs are alternated inside every repetition, `steps` calls between two
device synchronisations; the median, minimum and maximum over the repetitions are recorded with V and F.  The march leg is one
ego_march_density of 4096 rays x 512 samples (the same 18 taps per sample as a node of the field): `field_nodes_per_s` over
`march_samples_per_s` is a recorded ratio, not a pass mark.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of this tool
of its own.  Without a device the tool fails; it has no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
MARCH = (4096, 512)


def summary(v) -> dict:
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), n=len(v))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="calls per leg and repetition")
    ap.add_argument("--box", type=int, default=256, help="nodes per axis of the box lattice")
    ap.add_argument("--panorama", type=int, nargs=3, default=(128, 512, 1024), help="radii, H, W of the panorama lattice")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r19", "mesh.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("tools/bench_mesh.py needs a HIP device: a time from anything else says nothing", file=sys.stderr)
        return 1
    from egonerf_amd import _lib, geometry, synth
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig()
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), dev)
    c = np.asarray(model.coordinates.center.tolist(), np.float64)
    near, far = float(cfg.near), float(cfg.far)
    lattices = {
        f"box_{a.box}^3": geometry.box_lattice(c - 0.5 * far * np.array([1.0, 0.97, 1.03]), c + 0.5 * far * np.array([1.02, 1.0, 0.98]), (a.box,) * 3),
        "panorama_" + "x".join(map(str, a.panorama)): geometry.panorama_lattice(a.panorama[1], a.panorama[2],
                                                                             geometry.geometric_radii(max(near, 1e-2), far, a.panorama[0], dev)),
    }
    rays = torch.from_numpy(synth.make_rays(MARCH[0], seed=1)).to(dev)
    doc = dict(tool="tools/bench_mesh.py", device=torch.cuda.get_device_name(0), scene="synth.SceneConfig(), seed 1234", grid=list(cfg.grid),
               steps_per_leg=a.steps, reps=a.reps, march_shape=list(MARCH), lattices={})
    lib, centre = _lib.load(), model.coordinates.center.tolist()
    for name, lat in lattices.items():
        with torch.no_grad():
            values = geometry.lattice_field(model, lat)
            level = float(values.kthvalue(int(0.9 * lat.count)).values)
            L = lat.struct(centre)
            nbytes = int(lib.ego_mesh_workspace_bytes(L))
            ws, counts = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
            st = _lib.stream_handle()
            count = lambda: _lib.check(lib.ego_mesh_count(L, values.data_ptr(), level, ws.data_ptr(), nbytes, counts.data_ptr(), st), "ego_mesh_count")
            count()
            V, F = (int(v) for v in counts.tolist())
            vertices, faces = torch.empty(V, 3, device=dev), torch.empty(F, 3, dtype=torch.int32, device=dev)
            legs = {
                "field": lambda: geometry.lattice_field(model, lat),
                "count": count,
                "emit": lambda: _lib.check(lib.ego_mesh_emit(L, values.data_ptr(), level, ws.data_ptr(), V, F, vertices.data_ptr(), faces.data_ptr(), st),
                                           "ego_mesh_emit"),
                "point_gradients": lambda: geometry.point_gradient(model, vertices, True),
                "march": lambda: geometry.march_samples(model, rays, n_coarse=MARCH[1]),
            }
            for leg in legs.values():   # every shape the timed window uses, twice
                leg(); leg()
            torch.cuda.synchronize()
            times = {k: [] for k in legs}
            for _ in range(a.reps):
                for leg_name, leg in legs.items():
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        leg()
                    torch.cuda.synchronize()
                    times[leg_name].append((time.perf_counter() - t0) / a.steps * 1e3)
            t0 = time.perf_counter()
            whole = geometry.extract_mesh(model, lat, level)
            torch.cuda.synchronize()
            end_to_end = (time.perf_counter() - t0) * 1e3
            assert whole.vertices.shape[0] == V and whole.faces.shape[0] == F
            ms = {k: summary(v) for k, v in times.items()}
            nodes_per_s = lat.count / (ms["field"]["median"] * 1e-3)
            samples_per_s = MARCH[0] * MARCH[1] / (ms["march"]["median"] * 1e-3)
            doc["lattices"][name] = dict(n=list(lat.n), nodes=lat.count, level=level, V=V, F=F, workspace_bytes=nbytes, ms_per_call=ms,
                                         extract_mesh_with_normals_ms_one_call=end_to_end, field_nodes_per_s=nodes_per_s,
                                         march_samples_per_s=samples_per_s, field_over_march=nodes_per_s / samples_per_s)
            del values, ws, vertices, faces, whole
    print(json.dumps(doc, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
