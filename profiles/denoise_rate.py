"""Time of the denoiser (gi_denoise_device) on one GPU, beside the progressive pass its preview competes with.

For the Cornell box (the scene of C3), each frame size (1920 x 1080 and 2048 x 2048) and each focal length (the
scene's own, at which the box covers under a tenth of these frames and every other pixel passes through, and
one at which it fills most of the frame): the
frame's feature buffers (gi_render_aov_device) and the first 1-spp pass of a 4-spp, depth-4 progressive Mode X
frame are made once; then gi_denoise_device over them with 1 to 5 levels, with and without the albedo stop, at
sigma_c = 0.5 (one sample so far), the other parameters the defaults.  Each call is timed with HIP events on
its stream: warm-up calls of each, then --calls timed rounds (20 at least), a round being one call of every
configuration in turn (they alternate, so they share whatever else the device is doing); the report is the
median and the range, per call and per level.

The pure-stream time of a call is what a copy of the bytes it must move would take: k_dn_prep reads t and the
normal (and the albedo) and writes a 64-byte guide record (and a 32-byte albedo record) per pixel; every level
reads the guide record (and the albedo record) and the colour once and writes the colour (the last one also the
8-bit frame) -- divided by COPY_BYTES_PER_S of profiles/aov_rate.py.  `times_the_floor` is the call's median
over that time.  The 1-spp pass: every pass of --frames progressive frames (4 passes each), timed the same way.
One JSON line per measurement.

    python profiles/denoise_rate.py [--frames-of 1920x1080,2048x2048] [--focals scene,0.6] [--calls K] [--warmup W] [--out FILE]
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

SPP, DEPTH, SEED = 4, 4, 1


def stream_bytes_per_pixel(levels, stop):
    """(prep, per level, extra of the last level) bytes read once and written per pixel."""
    prep = 8 + 24 + 64 + ((24 + 32) if stop else 0)
    level = 64 + (32 if stop else 0) + 24 + 24
    return prep, level, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-of", default="1920x1080,2048x2048")
    ap.add_argument("--focals", default="scene,0.6", help="camera focal lengths: the scene's own (the box covers a small part of the "
                    "frame: most pixels pass through) and one at which the box fills most of it")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=6, help="progressive frames (4 passes each) for the pass time")
    ap.add_argument("--label", default="direct", help="labels the level kernel's form of the library under test (GI_LIB selects a build)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.calls < 20 or a.frames * SPP < 20:
        ap.error("--calls and --frames x 4: at least 20 timed calls")
    import torch
    from importlib import import_module
    gi = import_module("2019global_amd")
    S = import_module("2019global_amd.scenes")
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    sc = S.named_scene("cornell")
    dev = gi.DeviceScene.from_scene(sc)
    lines = []
    for size, focal in [(s, f) for s in a.frames_of.split(",") for f in a.focals.split(",")]:
        w, h = (int(v) for v in size.split("x"))
        focal = sc.focal if focal == "scene" else float(focal)
        cam = gi.Camera(sc.cam_pos, sc.cam_look, focal)
        n = w * h
        f64 = lambda k: torch.empty(k * n, dtype=torch.float64, device="cuda")   # noqa: E731
        rgb, t, nrm, alb, out = f64(3), f64(1), f64(3), f64(3), f64(3)
        out8 = torch.empty(3 * n, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        kw = dict(mode=gi.MODE_X, spp=SPP, depth=DEPTH, seed=SEED, stream=st.cuda_stream)
        # the 1-spp passes (the last frame's first pass stays in rgb: the denoiser's input)
        pev = []
        with torch.cuda.stream(st):
            dev.render_aov_device(cam, w, h, d_t=t.data_ptr(), d_normal=nrm.data_ptr(), d_albedo=alb.data_ptr(), stream=st.cuda_stream)
            for fr in range(a.frames + 1):
                for s in range(SPP):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    dev.render_device(cam, sc.light, w, h, out.data_ptr() if s else rgb.data_ptr(), samples=(s, s + 1), **kw)
                    e1.record(st)
                    if fr:   # (the first frame warms up)
                        pev.append((e0, e1))
        st.synchronize()
        pass_ms = np.array([e0.elapsed_time(e1) for e0, e1 in pev])
        valid = float((t < float("inf")).double().mean().item())
        cfgs = [(k, stop) for k in (1, 2, 3, 4, 5) for stop in (True, False)]
        scratch = torch.empty(max(gi.denoise_scratch_bytes(w, h, levels=k, albedo_stop=stop) for k, stop in cfgs), dtype=torch.uint8,
                              device="cuda")

        def call(k, stop):
            gi.denoise_device(cam, w, h, rgb.data_ptr(), t.data_ptr(), nrm.data_ptr(), alb.data_ptr() if stop else 0, scratch.data_ptr(),
                              scratch.numel(), d_out_rgb=out.data_ptr(), d_out_rgb8=out8.data_ptr(), levels=k, sigma_c=0.5,
                              albedo_stop=stop, stream=st.cuda_stream)
        ev = {c: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)] for c in cfgs}
        with torch.cuda.stream(st):
            for _ in range(a.warmup):
                for c in cfgs:
                    call(*c)
            for r in range(a.calls):
                for c in cfgs:
                    e0, e1 = ev[c][r]
                    e0.record(st)
                    call(*c)
                    e1.record(st)
        st.synchronize()
        for (k, stop) in cfgs:
            ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev[(k, stop)]])
            med = float(np.median(ms))
            prep_b, level_b, last_b = stream_bytes_per_pixel(k, stop)
            floor_ms = n * (prep_b + k * level_b + last_b) / COPY_BYTES_PER_S * 1e3
            rec = {"scene": "cornell", "form": a.label, "focal": focal, "frame": [w, h], "n": n, "valid_fraction": round(valid, 4), "levels": k,
                   "albedo_stop": stop, "calls": a.calls, "ms_median": round(med, 4), "ms_min": round(float(ms.min()), 4),
                   "ms_max": round(float(ms.max()), 4), "ms_per_level_median": round(med / k, 4),
                   "stream_bytes_per_pixel": prep_b + k * level_b + last_b, "stream_floor_ms": round(floor_ms, 4),
                   "times_the_floor": round(med / floor_ms, 2),
                   "pass_1spp_ms_median": round(float(np.median(pass_ms)), 4), "pass_1spp_ms_min": round(float(pass_ms.min()), 4),
                   "pass_1spp_ms_max": round(float(pass_ms.max()), 4), "pass_calls": len(pass_ms),
                   "times_the_pass": round(med / float(np.median(pass_ms)), 2)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        del rgb, t, nrm, alb, out, out8, scratch
    dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
