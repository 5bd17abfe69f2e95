"""Rate of the radiance query (gi_radiance_device) and its two companions on one GPU, beside their yardsticks.

For each scene (the Cornell box -- C3's frame -- and soup100000) a 1920 x 1080 frame at 8 spp and depth 8: 16.6 M
records resident in device memory, made once by gi_sample_rays_device (jittered, no lens).  Measured in the same run,
the calls taking turns within every round (HIP events on one stream; warm-up rounds, then --rounds timed ones, the
report is the median and the range over the rounds):
  radiance     gi_radiance_device over the prepared records;
  render       gi_render_device of the same frame, spp and depth: the same paths through the render's own kernels
               (classify, k_seg or its kin, reduce) -- the rows are those radiance writes, bit for bit;
  copy_rad     a device copy of the call's bytes: 64 + 16 read and 24 written per record;
  sample_rays  gi_sample_rays_device, and copy_sample: a copy of the 80 bytes per record it writes;
  resolve      gi_resolve_samples_device (rgb and rgb8), and copy_resolve: a copy of the 24 bytes per record it reads.
A copy of b bytes moves b in and b out, so copy_rad copies (80 + 24) / 2 bytes per record and the others half
their bytes: each copy's traffic equals its call's.  One JSON line per measurement, ratios against the yardsticks in
the summary line of each scene.

    python profiles/radiance_rate.py [--rounds K] [--warmup W] [--scenes cornell,soup100000] [--spp 8] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, DEPTH, SEED = 1920, 1080, 8, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="cornell,soup100000")
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10 timed rounds")
    import torch
    from importlib import import_module
    gi = import_module("2019global_amd")
    S = import_module("2019global_amd.scenes")
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    spp, n_pix = a.spp, W * H
    n = n_pix * spp
    lines = []
    f64 = dict(dtype=torch.float64, device="cuda")
    rays, ids = torch.empty(8 * n, **f64), torch.empty(2 * n, dtype=torch.int64, device="cuda")
    rows, rgb = torch.empty(3 * n, **f64), torch.empty(3 * n_pix, **f64)
    rgb8 = torch.empty(3 * n_pix, dtype=torch.uint8, device="cuda")
    frame, frame8 = torch.empty(3 * n_pix, **f64), torch.empty(3 * n_pix, dtype=torch.uint8, device="cuda")
    src, dst = torch.empty(52 * n, dtype=torch.uint8, device="cuda"), torch.empty(52 * n, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    q = st.cuda_stream
    for name in a.scenes.split(","):
        sc = S.named_scene(name)
        dev = gi.DeviceScene.from_scene(sc)
        cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
        var = dev.kat_x_variant(0)
        kw = dict(mode=gi.MODE_X, spp=spp, depth=DEPTH, seed=SEED)
        calls = {
            "radiance": lambda: dev.radiance_device(n, rays.data_ptr(), rows.data_ptr(), sc.light, DEPTH, d_ids=ids.data_ptr(),
                                                    seed=SEED, stream=q),
            "render": lambda: dev.render_device(cam, sc.light, W, H, frame.data_ptr(), frame8.data_ptr(), stream=q, **kw),
            "copy_rad": lambda: dst[:52 * n].copy_(src[:52 * n], non_blocking=True),
            "sample_rays": lambda: gi.sample_rays_device(cam, W, H, rays.data_ptr(), ids.data_ptr(), samples=spp, seed=SEED, stream=q),
            "copy_sample": lambda: dst[:40 * n].copy_(src[:40 * n], non_blocking=True),
            "resolve": lambda: gi.resolve_samples_device(n_pix, spp, rows.data_ptr(), rgb.data_ptr(), rgb8.data_ptr(), stream=q),
            "copy_resolve": lambda: dst[:12 * n].copy_(src[:12 * n], non_blocking=True),
        }
        ms = {k: [] for k in calls}
        with torch.cuda.stream(st):
            calls["sample_rays"]()
            for r in range(a.warmup + a.rounds):
                ev = {}
                for k, fn in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    ev[k] = (e0, e1)
                st.synchronize()
                if r >= a.warmup:
                    for k, (e0, e1) in ev.items():
                        ms[k].append(e0.elapsed_time(e1))
        # the timed calls computed the same thing: radiance's resolved rows are the render's frame
        same = bool((rgb == frame).all().item() and (rgb8 == frame8).all().item())
        lit = round(float((rows.view(-1, 3) != 0).any(1).double().mean().item()), 4)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, v in ms.items():
            rec = {"scene": name, "variant": "".join(x for x, y in var.items() if y) or "HBM", "call": k, "records": n, "spp": spp,
                   "depth": DEPTH, "rounds": a.rounds, "ms_median": round(med[k], 4), "ms_min": round(float(min(v)), 4),
                   "ms_max": round(float(max(v)), 4), "mrecords_per_s": round(n / med[k] * 1e-3, 1)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        rec = {"scene": name, "summary": True, "resolved_rows_equal_the_render": same, "records_with_radiance": lit,
               "radiance_over_render": round(med["radiance"] / med["render"], 3),
               "radiance_over_copy": round(med["radiance"] / med["copy_rad"], 2),
               "sample_rays_over_copy": round(med["sample_rays"] / med["copy_sample"], 2),
               "resolve_over_copy": round(med["resolve"] / med["copy_resolve"], 2),
               "three_calls_over_render": round((med["sample_rays"] + med["radiance"] + med["resolve"]) / med["render"], 3)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
