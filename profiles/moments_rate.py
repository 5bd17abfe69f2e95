"""Time of the sample moments (gi_frame_moments_device) and of the variance-guided denoiser
(gi_denoise_var_device) on one GPU, each beside its yardstick.

The Cornell box at 1920 x 1080, 64 spp, depth 4, for each focal length (the scene's own, at which the box covers
under a tenth of the frame, and one at which it fills most of it): one render leaves the retained frame; then
  moments      gi_frame_moments_device of the whole frame into mean and var (k_x_moments_fill + k_x_moments);
  denoise_var  gi_denoise_var_device over mean, var and the frame's feature buffers at 1 and 4 levels, and
               gi_denoise_device at the same levels on the same planes -- its yardstick, from the same build.
Each call is timed with HIP events on its stream: --warmup calls of each, then --calls timed rounds (20 at least),
a round being one call of every configuration in turn; the report is the median and the range.

The pure-stream time of a call is what a copy of the bytes it must move would take, over COPY_BYTES_PER_S of
profiles/aov_rate.py: the moments read every listed pixel's n rows once (24 n bytes; the second pass over them is
the kernel's own business) and write mean and var for every pixel; the denoiser as profiles/denoise_rate.py counts
it, with the variance planes (24 + 24 bytes per level), the g plane (8 written and 8 read per level) and the input
variance.  `times_the_floor` is the median over that time.

The moments' yardstick is k_x_reduce on the same frame, which reads the same rows once; it runs inside the render,
so its time comes from a kernel trace of this script:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python profiles/moments_rate.py --calls 20
    python profiles/moments_rate.py --stats-csv DIR/.../run_kernel_stats.csv
the second command prints the average of k_x_reduce, k_x_moments and k_x_moments_fill from the trace (no GPU).
--label names the k_x_moments form of the library under test (GI_LIB selects a build: GI_MOMENTS_LDS=0|1).
One JSON line per measurement.

    python profiles/moments_rate.py [--frame 1920x1080] [--focals scene,0.6] [--spp 64] [--calls K] [--warmup W] [--label L] [--out FILE]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from aov_rate import COPY_BYTES_PER_S   # noqa: E402

DEPTH, SEED = 4, 1


def stats_csv(path):
    """The moments kernels and their yardstick from a rocprofv3 kernel-stats CSV."""
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        for k in ("k_x_reduce", "k_x_moments_fill", "k_x_moments"):
            if k + "(" in name or name.endswith(k) or ("::" + k + " ") in name + " ":
                print(json.dumps({"kernel": k, "calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                  "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}))
                break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", default="1920x1080")
    ap.add_argument("--focals", default="scene,0.6")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="lds", help="labels the k_x_moments form of the library under test")
    ap.add_argument("--stats-csv", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.stats_csv:
        return stats_csv(a.stats_csv)
    if a.calls < 20:
        ap.error("--calls: at least 20 timed calls")
    import torch
    from importlib import import_module
    gi = import_module("2019global_amd")
    S = import_module("2019global_amd.scenes")
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    sc = S.named_scene("cornell")
    dev = gi.DeviceScene.from_scene(sc)
    w, h = (int(v) for v in a.frame.split("x"))
    n, spp = w * h, a.spp
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    for focal in a.focals.split(","):
        focal = sc.focal if focal == "scene" else float(focal)
        cam = gi.Camera(sc.cam_pos, sc.cam_look, focal)
        f64 = lambda k: torch.empty(k * n, dtype=torch.float64, device="cuda")   # noqa: E731
        rgb, mean, var, t, nrm, alb, out, ovar = f64(3), f64(3), f64(3), f64(1), f64(3), f64(3), f64(3), f64(3)
        out8 = torch.empty(3 * n, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            dev.render_aov_device(cam, w, h, d_t=t.data_ptr(), d_normal=nrm.data_ptr(), d_albedo=alb.data_ptr(), stream=st.cuda_stream)
            for _ in range(2):   # (the render runs k_x_reduce: the kernel trace's yardstick)
                dev.render_device(cam, sc.light, w, h, rgb.data_ptr(), mode=gi.MODE_X, spp=spp, depth=DEPTH, seed=SEED, stream=st.cuda_stream)
        st.synchronize()
        assert dev.frame_samples_info() == dict(w=w, h=h, n=spp, spp=spp)
        valid = float((t < float("inf")).double().mean().item())

        def moments():
            dev.frame_moments_device(w, h, d_mean=mean.data_ptr(), d_var=var.data_ptr(), stream=st.cuda_stream)
        levels = (1, 4)
        scratch = torch.empty(max(gi.denoise_var_scratch_bytes(w, h, levels=k) for k in levels), dtype=torch.uint8, device="cuda")

        def dn_var(k):
            gi.denoise_var_device(cam, w, h, mean.data_ptr(), var.data_ptr(), t.data_ptr(), nrm.data_ptr(), alb.data_ptr(), scratch.data_ptr(),
                                  scratch.numel(), d_out_rgb=out.data_ptr(), d_out_var=ovar.data_ptr(), d_out_rgb8=out8.data_ptr(), levels=k,
                                  stream=st.cuda_stream)

        def dn_fixed(k):
            gi.denoise_device(cam, w, h, mean.data_ptr(), t.data_ptr(), nrm.data_ptr(), alb.data_ptr(), scratch.data_ptr(), scratch.numel(),
                              d_out_rgb=out.data_ptr(), d_out_rgb8=out8.data_ptr(), levels=k, sigma_c=0.5 / np.sqrt(spp), stream=st.cuda_stream)
        calls = {"moments": moments}
        for k in levels:
            calls["denoise_var/%d" % k] = lambda k=k: dn_var(k)
            calls["denoise/%d" % k] = lambda k=k: dn_fixed(k)
        ev = {c: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)] for c in calls}
        with torch.cuda.stream(st):
            for _ in range(a.warmup):
                for c in calls.values():
                    c()
            for r in range(a.calls):
                for name, c in calls.items():
                    e0, e1 = ev[name][r]
                    e0.record(st)
                    c()
                    e1.record(st)
        st.synchronize()
        listed = float((mean.view(n, 3) != 0).any(1).double().mean().item())   # (a lower bound: listed pixels that are not black)
        med = {}
        for name in calls:
            ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev[name]])
            med[name] = float(np.median(ms))
            rec = {"scene": "cornell", "focal": focal, "frame": [w, h], "spp": spp, "call": name, "calls": a.calls,
                   "ms_median": round(med[name], 4), "ms_min": round(float(ms.min()), 4), "ms_max": round(float(ms.max()), 4),
                   "valid_fraction": round(valid, 4)}
            if name == "moments":
                by = n * (listed * 24 * spp + 48)
                rec.update(form=a.label, nonblack_fraction=round(listed, 4), stream_bytes=int(by))
            else:
                kind, k = name.split("/")
                k = int(k)
                per_px = (8 + 24 + 64 + 24 + 32) + k * (64 + 32 + 24 + 24) + 3
                if kind == "denoise_var":
                    per_px += k * (24 + 24 + 8 + 8 + 24)   # the variance in and out, g written and read, the prefilter's read of V
                by = n * per_px
                rec.update(levels=k, stream_bytes=int(by))
            floor_ms = by / COPY_BYTES_PER_S * 1e3
            rec.update(stream_floor_ms=round(floor_ms, 4), times_the_floor=round(med[name] / floor_ms, 2))
            emit(rec)
        for k in levels:
            emit({"scene": "cornell", "focal": focal, "frame": [w, h], "levels": k,
                  "denoise_var_over_denoise": round(med["denoise_var/%d" % k] / med["denoise/%d" % k], 3)})
        del rgb, mean, var, t, nrm, alb, out, ovar, out8, scratch
    dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
