"""Ray rate of the batched device queries (gi_intersect_device, gi_occluded_device) on one GPU.

For each scene (the Cornell box -- the scene of C3 -- and soup100000) and each ray set, 2^22 rays
resident in device memory:
  camera : the pixel rays of the scene's own camera over a 1920 x 1080 frame, in row order (coherent),
           repeated to the ray count;
  random : seeded random rays through the bounds (origins within 1.5 half-extents of the centre,
           aimed at uniform points of the bounds).
Each call is timed with HIP events on its stream: warm-up calls, then --calls timed ones (20 at least);
the report is the median and the range, in rays per second.  Beside it stands the stream floor of the
call: the bytes a ray costs if nothing but its record were read and its outputs written (64 + 40 for
intersect with every output, 64 + 4 for occluded) at the 6.29 TB/s a device-to-device copy reaches on
this part -- how far the kernel is from being a pure stream.  One JSON line per measurement.

    python profiles/cast_rate.py [--rays N] [--calls K] [--warmup W] [--scenes cornell,soup100000] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_BYTES_PER_S = 6.29e12   # measured device-to-device copy rate of the MI355X (read + write counted)


def primary_dirs(sc, w, h):
    """raytracer.h:26-30, 41-43 (the kernels' make_cam / primary_dir): the w x h pixel directions, row order."""
    pos, look = np.array(sc.cam_pos, np.float64), np.array(sc.cam_look, np.float64)
    f = look - pos
    f = f / np.sqrt((f * f).sum())
    up = np.array([0.0, 0.0, 1.0])
    left = np.cross(up, f)
    left = left / np.sqrt((left * left).sum())
    r = 0.0002
    tl = (((pos + sc.focal * f) + ((left * float(w)) * 0.5) * r) + ((up * float(w)) * 0.5) * r) - pos
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = (tl[None, None, :] - (left[None, None, :] * x[:, :, None]) * r) - (up[None, None, :] * y[:, :, None]) * r
    return pos, d.reshape(-1, 3)


def bounds(sc, S):
    pts = []
    for e in sc.entities:
        if e.kind == S.IMP_TRIANGLE:
            pts.append(np.array(e.args[:9]).reshape(3, 3))
    p = np.concatenate(pts)
    return p.min(0), p.max(0)


def ray_sets(sc, S, n, seed):
    pos, dirs = primary_dirs(sc, 1920, 1080)
    cam = np.zeros((n, 8))
    cam[:, 0:3] = pos
    cam[:, 3:6] = dirs[np.arange(n) % len(dirs)]
    cam[:, 6] = np.inf
    lo, hi = bounds(sc, S)
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(seed)
    rnd = np.zeros((n, 8))
    rnd[:, 0:3] = c + (2.0 * rng.random((n, 3)) - 1.0) * (1.5 * half)
    aim = lo + rng.random((n, 3)) * (hi - lo)
    d = aim - rnd[:, 0:3]
    rnd[:, 3:6] = d / np.sqrt((d * d).sum(1, keepdims=True))
    rnd[:, 6] = np.inf
    return {"camera": cam, "random": rnd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=2 ** 22)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="cornell,soup100000")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls: at least 20 timed calls")
    import torch
    from importlib import import_module
    gi = import_module("2019global_amd")
    S = import_module("2019global_amd.scenes")
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n = a.rays
    lines = []
    for name in a.scenes.split(","):
        sc = S.named_scene(name)
        dev = gi.DeviceScene.from_scene(sc)
        var = dev.kat_x_variant(0)
        t = torch.empty(n, dtype=torch.float64, device="cuda")
        prim = torch.empty(n, dtype=torch.int32, device="cuda")
        ent = torch.empty(n, dtype=torch.int32, device="cuda")
        nrm = torch.empty(3 * n, dtype=torch.float64, device="cuda")
        occ = torch.empty(n, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        for set_name, rays_h in ray_sets(sc, S, n, 2019).items():
            rays = torch.from_numpy(rays_h).cuda()
            torch.cuda.synchronize()
            calls = {
                "intersect": (64 + 40, lambda: dev.intersect_device(n, rays.data_ptr(), t.data_ptr(), prim.data_ptr(), ent.data_ptr(),
                                                                    nrm.data_ptr(), stream=st.cuda_stream)),
                "occluded": (64 + 4, lambda: dev.occluded_device(n, rays.data_ptr(), occ.data_ptr(), stream=st.cuda_stream)),
            }
            for call, (bytes_per_ray, fn) in calls.items():
                with torch.cuda.stream(st):
                    for _ in range(a.warmup):
                        fn()
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
                    for e0, e1 in ev:
                        e0.record(st)
                        fn()
                        e1.record(st)
                st.synchronize()
                ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
                hits = int((prim >= 0).sum().item()) if call == "intersect" else int(occ.sum().item())
                floor_ms = n * bytes_per_ray / COPY_BYTES_PER_S * 1e3
                rec = {"scene": name, "variant": "".join(k for k, v in var.items() if v) or "HBM", "rays": set_name, "call": call,
                       "n": n, "calls": a.calls, "hit_fraction": round(hits / n, 4),
                       "ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
                       "ms_max": round(float(ms.max()), 4),
                       "grays_per_s_median": round(n / float(np.median(ms)) * 1e-6, 3),
                       "grays_per_s_range": [round(n / float(ms.max()) * 1e-6, 3), round(n / float(ms.min()) * 1e-6, 3)],
                       "bytes_per_ray": bytes_per_ray, "stream_floor_ms": round(floor_ms, 4),
                       "stream_floor_grays_per_s": round(COPY_BYTES_PER_S / bytes_per_ray * 1e-9, 2),
                       "times_the_floor": round(float(np.median(ms)) / floor_ms, 2)}
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
            del rays
        dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
