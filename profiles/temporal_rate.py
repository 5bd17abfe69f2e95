"""Time of the temporal accumulation (gi_temporal_device) on one GPU, beside one level of the denoiser and a copy of
the bytes it must move.

For the Cornell box (the scene of C3) at 1920 x 1080 and each focal length (the scene's own, at which the box covers
under a tenth of the frame and every other pixel passes through, and one at which it fills most of the frame): a
4-spp, depth-4 Mode X frame, its sample moments and its feature buffers are made for the camera and for a camera
shifted sideways by about --shift-pixels pixels at the middle of the box (15 away); the first camera's planes, with len = 4 everywhere, are the
history.  Then gi_temporal_device with and without the variance, with and without the prim stop, for the identical
camera (current = history: every tap of a pixel is accepted) and for the shifted one, and one level of
gi_denoise_device over the current planes.  Each call is timed with HIP events on its stream: warm-up calls of each,
then --calls timed rounds (20 at least), a round being one call of every configuration in turn (they alternate, so
they share whatever else the device is doing); the report is the median and the range.

The pure-stream time of a call is what a copy of the bytes it must move would take.  Per pixel the call reads the
current rgb, t and normal (56 B), the history's rgb, t, normal and len once (60 B: neighbouring pixels share their
taps) and writes rgb and len (28 B); the variance adds 24 B to each of the three, the prim stop 4 B to both reads.
`stream_floor_ms` divides them by COPY_BYTES_PER_S of profiles/aov_rate.py, as the other rate scripts do;
`copy_ms_median` is a device-to-device copy of half as many bytes (read once, written once: the same traffic), timed in
the same rounds (with the variance and without, at the prim stop's bytes; scaled by the bytes without it).
`times_the_floor` and `times_the_copy` are the call's median over each.  One JSON line per
measurement.

    python profiles/temporal_rate.py [--frame 1920x1080] [--focals scene,0.6] [--shift-pixels 3] [--calls K] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from aov_rate import COPY_BYTES_PER_S   # noqa: E402

SPP, DEPTH = 4, 4


def stream_bytes_per_pixel(var, prim):
    """Bytes read once and written per pixel."""
    return (56 + 60 + 28) + (72 if var else 0) + (8 if prim else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", default="1920x1080")
    ap.add_argument("--focals", default="scene,0.6")
    ap.add_argument("--shift-pixels", type=float, default=3.0, help="sideways translation of the shifted camera, in pixels at 15 units' distance")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    sc = S.named_scene("cornell")
    dev = gi.DeviceScene.from_scene(sc)
    w, h = (int(v) for v in a.frame.split("x"))
    n = w * h
    lines = []
    for focal in a.focals.split(","):
        focal = sc.focal if focal == "scene" else float(focal)
        shift = a.shift_pixels * 0.0002 / focal * 15.0   # (0.0002: the pixel pitch on the image plane at distance focal)
        cams = {"identical": gi.Camera(sc.cam_pos, sc.cam_look, focal),
                "shifted": gi.Camera(np.add(sc.cam_pos, (0.0, shift, 0.0)), np.add(sc.cam_look, (0.0, shift, 0.0)), focal)}
        st = torch.cuda.Stream()
        f64 = lambda k: torch.empty(k * n, dtype=torch.float64, device="cuda")   # noqa: E731
        i32 = lambda: torch.empty(n, dtype=torch.int32, device="cuda")   # noqa: E731
        frame = f64(3)
        planes = {}
        for k, (name, cam) in enumerate(cams.items()):
            p = dict(rgb=f64(3), var=f64(3), t=f64(1), normal=f64(3), albedo=f64(3), prim=i32())
            dev.render_device(cam, sc.light, w, h, frame.data_ptr(), stream=st.cuda_stream, mode=gi.MODE_X, spp=SPP, depth=DEPTH, seed=1 + k)
            dev.frame_moments_device(w, h, d_mean=p["rgb"].data_ptr(), d_var=p["var"].data_ptr(), stream=st.cuda_stream)
            dev.render_aov_device(cam, w, h, d_t=p["t"].data_ptr(), d_normal=p["normal"].data_ptr(), d_albedo=p["albedo"].data_ptr(),
                                  d_prim=p["prim"].data_ptr(), stream=st.cuda_stream)
            planes[name] = p
        st.synchronize()
        hist_len = torch.full((n,), SPP, dtype=torch.int32, device="cuda")
        out_rgb, out_var, out_len = f64(3), f64(3), i32()
        names = ("rgb", "var", "t", "normal", "prim")
        d_hist = dict({k: planes["identical"][k].data_ptr() for k in names}, len=hist_len.data_ptr())
        valid = float((planes["identical"]["t"] < float("inf")).double().mean().item())
        scratch = torch.empty(gi.denoise_scratch_bytes(w, h, levels=1), dtype=torch.uint8, device="cuda")
        copy_src = {v: torch.empty(stream_bytes_per_pixel(v, True) * n // 2, dtype=torch.uint8, device="cuda") for v in (True, False)}
        copy_dst = {v: torch.empty_like(t) for v, t in copy_src.items()}

        def temporal(pair, var, prim):
            cur = planes[pair]
            gi.temporal_device(cams[pair], cams["identical"], w, h,
                               {k: cur[k].data_ptr() for k in names if (k != "var" or var) and (k != "prim" or prim)},
                               {k: v for k, v in d_hist.items() if (k != "var" or var) and (k != "prim" or prim)},
                               d_out_rgb=out_rgb.data_ptr(), d_out_var=out_var.data_ptr() if var else 0, d_out_len=out_len.data_ptr(),
                               prim_stop=prim, stream=st.cuda_stream)

        def denoise_level():
            cur = planes["shifted"]
            gi.denoise_device(cams["shifted"], w, h, cur["rgb"].data_ptr(), cur["t"].data_ptr(), cur["normal"].data_ptr(), cur["albedo"].data_ptr(),
                              scratch.data_ptr(), scratch.numel(), d_out_rgb=out_rgb.data_ptr(), levels=1, sigma_c=0.25, stream=st.cuda_stream)
        calls = {("temporal", pair, var, prim): (lambda pair=pair, var=var, prim=prim: temporal(pair, var, prim))
                 for pair in cams for var in (True, False) for prim in (True, False)}
        calls[("denoise_1_level",)] = denoise_level
        for v in (True, False):
            calls[("copy", v)] = lambda v=v: copy_dst[v].copy_(copy_src[v])
        ev = {c: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)] for c in calls}
        with torch.cuda.stream(st):
            for _ in range(a.warmup):
                for f in calls.values():
                    f()
            for r in range(a.calls):
                for c, f in calls.items():
                    e0, e1 = ev[c][r]
                    e0.record(st)
                    f()
                    e1.record(st)
        st.synchronize()
        ms = {c: np.array([e0.elapsed_time(e1) for e0, e1 in ev[c]]) for c in calls}
        accepted = {}
        for pair in cams:   # what the last call of the pair left: the share of valid pixels that found history
            temporal(pair, True, True)
            st.synchronize()
            accepted[pair] = float((out_len > 1).double().sum().item()) / max(1.0, float((planes[pair]["t"] < float("inf")).double().sum().item()))
        base = {"scene": "cornell", "focal": focal, "frame": [w, h], "n": n, "valid_fraction": round(valid, 4), "calls": a.calls}
        for c in calls:
            med = float(np.median(ms[c]))
            rec = dict(base, call=c[0], ms_median=round(med, 4), ms_min=round(float(ms[c].min()), 4), ms_max=round(float(ms[c].max()), 4))
            if c[0] == "temporal":
                _, pair, var, prim = c
                b = stream_bytes_per_pixel(var, prim)
                floor_ms = n * b / COPY_BYTES_PER_S * 1e3
                copy_med = float(np.median(ms[("copy", var)])) * b / stream_bytes_per_pixel(var, True)
                rec.update(camera=pair, variance=var, prim_stop=prim, accepted_fraction_of_valid=round(accepted[pair], 4),
                           stream_bytes_per_pixel=b, stream_floor_ms=round(floor_ms, 4), times_the_floor=round(med / floor_ms, 2),
                           copy_ms_median=round(copy_med, 4), times_the_copy=round(med / copy_med, 2),
                           gbytes_per_s=round(n * b / med * 1e-6, 1))
            elif c[0] == "copy":
                rec.update(variance=c[1], bytes=int(copy_src[c[1]].numel()) * 2, gbytes_per_s=round(copy_src[c[1]].numel() * 2 / med * 1e-6, 1))
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        del planes, frame, out_rgb, out_var, out_len, scratch, copy_src, copy_dst
    dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
