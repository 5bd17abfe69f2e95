"""Pixel rate of the feature buffers (gi_render_aov_device) on one GPU, beside the ray query they replace.

For each scene (the Cornell box -- the scene of C3 -- and soup100000), its own camera and a 2048 x 2048
frame, 2^22 pixels (profiles/cast_rate.py's ray count), three calls on one stream:
  intersect : gi_intersect_device with all four outputs over the frame's pixel rays, resident in device
              memory (written once by gi_camera_rays_device) -- the reference: what a caller had before;
  aov4      : gi_render_aov_device with t, prim, entity, normal -- the same queries and the same 40 bytes
              written per pixel, without the 64-byte ray record read;
  aov6      : gi_render_aov_device with every output (72 bytes written per pixel).
Each call is timed with HIP events on its stream: warm-up calls of each, then --calls timed rounds
(20 at least), a round being one call of each in turn (the three alternate, so they share whatever else
the device is doing); the report is the median and the range.  The bound: aov4's median may exceed the
reference's median by no more than the reference's own observed range (max - min).  One JSON line per
measurement.  --mapping labels the lane-to-pixel mapping of the library under test (GI_LIB selects a build):
the results of record compare the kernel's row mapping with an 8 x 8 tile build that was removed after it
lost (DESIGN.md §9 "Feature buffers").

    python profiles/aov_rate.py [--size 2048] [--calls K] [--warmup W] [--scenes cornell,soup100000]
                                [--mapping rows] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_BYTES_PER_S = 6.29e12   # measured device-to-device copy rate of the MI355X (read + write counted)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="cornell,soup100000")
    ap.add_argument("--mapping", default="rows")
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
    w = h = a.size
    n = w * h
    lines = []
    for name in a.scenes.split(","):
        sc = S.named_scene(name)
        dev = gi.DeviceScene.from_scene(sc)
        cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
        var = dev.kat_x_variant(0)
        f64 = lambda k: torch.empty(k * n, dtype=torch.float64, device="cuda")   # noqa: E731
        i32 = lambda k: torch.empty(k * n, dtype=torch.int32, device="cuda")     # noqa: E731
        rays = f64(gi.RAY_DOUBLES)
        q = dict(t=f64(1), prim=i32(1), entity=i32(1), normal=f64(3))                          # the query's outputs
        o = dict(t=f64(1), normal=f64(3), albedo=f64(3), prim=i32(1), entity=i32(1), uv=i32(2))  # the feature buffers
        st = torch.cuda.Stream()
        gi.camera_rays_device(cam, w, h, rays.data_ptr(), stream=st.cuda_stream)
        four = {"d_" + k: o[k].data_ptr() for k in ("t", "prim", "entity", "normal")}
        six = {"d_" + k: v.data_ptr() for k, v in o.items()}
        calls = {
            "intersect": (64 + 40, lambda: dev.intersect_device(n, rays.data_ptr(), q["t"].data_ptr(), q["prim"].data_ptr(),
                                                                q["entity"].data_ptr(), q["normal"].data_ptr(), stream=st.cuda_stream)),
            "aov4": (40, lambda: dev.render_aov_device(cam, w, h, stream=st.cuda_stream, **four)),
            "aov6": (72, lambda: dev.render_aov_device(cam, w, h, stream=st.cuda_stream, **six)),
        }
        ev = {c: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
              for c in calls}
        with torch.cuda.stream(st):
            for _ in range(a.warmup):
                for _, fn in calls.values():
                    fn()
            for r in range(a.calls):
                for c, (_, fn) in calls.items():
                    e0, e1 = ev[c][r]
                    e0.record(st)
                    fn()
                    e1.record(st)
        st.synchronize()
        # the three calls answered the same pixels alike
        same = bool((q["prim"] == o["prim"]).all().item() and (q["entity"] == o["entity"]).all().item() and
                    (q["t"].view(torch.int64) == o["t"].view(torch.int64)).all().item() and
                    (q["normal"].view(torch.int64) == o["normal"].view(torch.int64)).all().item())
        hits = int((o["prim"] >= 0).sum().item())
        ms = {c: np.array([e0.elapsed_time(e1) for e0, e1 in ev[c]]) for c in calls}
        ref_med, ref_range = float(np.median(ms["intersect"])), float(ms["intersect"].max() - ms["intersect"].min())
        for c, (bytes_per_px, _) in calls.items():
            med = float(np.median(ms[c]))
            floor_ms = n * bytes_per_px / COPY_BYTES_PER_S * 1e3
            rec = {"scene": name, "variant": "".join(k for k, v in var.items() if v) or "HBM", "mapping": a.mapping, "call": c,
                   "frame": [w, h], "n": n, "calls": a.calls, "hit_fraction": round(hits / n, 4), "same_answers": same,
                   "ms_median": round(med, 4), "ms_min": round(float(ms[c].min()), 4), "ms_max": round(float(ms[c].max()), 4),
                   "gpix_per_s_median": round(n / med * 1e-6, 3),
                   "gpix_per_s_range": [round(n / float(ms[c].max()) * 1e-6, 3), round(n / float(ms[c].min()) * 1e-6, 3)],
                   "bytes_per_pixel": bytes_per_px, "stream_floor_ms": round(floor_ms, 4),
                   "times_the_floor": round(med / floor_ms, 2)}
            if c == "aov4":
                rec["bound_ms"] = round(ref_med + ref_range, 4)   # the reference's median + its own range
                rec["within_bound"] = bool(med <= ref_med + ref_range)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        del rays, q, o
        dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
