"""What adaptive sampling (gi_render_adaptive_device) costs and buys on one GPU.  One JSON line per measurement.

overhead   C3's frame (Cornell box, 1920 x 1080, depth 8, 64 spp) three ways, in interleaved rounds (one frame of
           each per round, so they share whatever else the device is doing): one shot; plain progressive passes of 8;
           adaptive passes of 8 with tol = 5e-324, min_samples = 2 (nothing but pixels of zero variance stops: the
           passes trace what the plain ones trace).  Every frame is timed with HIP events on its stream; the report is
           the median and the range over --rounds rounds after --warmup.  With GI_FLAG_TIME the passes also report
           their dominant kernel, so `other_ms_per_pass` = pass - kernel is what the passes after the first spend
           between the render kernels: k_x_adapt_fill, k_x_adapt_fold and two memsets (plain passes: k_x_classify and
           k_x_reduce).  Its pure-stream time: the bytes fold and fill must move -- per active entry its k rows
           (24 k B), the state read and written (48 + 48 + 4 B), the list entry read and written (4 + 4 B) and the
           planes given (rgb 24, the 8-bit frame 3); per slot of the frame the 4-byte state word fill reads -- over
           COPY_BYTES_PER_S of profiles/aov_rate.py.
           --plain-only skips the adaptive frames, and --tree DIR measures the package and library of another checkout
           (a built checkout of the parent commit): its one-shot and plain progressive figures, for the claim that
           k_seg is unchanged.
gain       On C3's scene and on C4's soup (100k triangles), 1920 x 1080, depth 8, at most 64 spp in passes of 8,
           min_samples 8: a sweep of tol, absolute and relative (y_floor 0.05).  Per setting the mean n over the
           frame, GI_STAT_RAYS, the frame's time (median of --rounds), and the mean squared error of the delivered
           frame against a 2048-spp frame of another seed; beside it the plain frame whose spp is nearest the mean n
           (a mean over the whole frame: the resolved pixels weigh in with n = 8) and the plain frame of equal
           GI_STAT_RAYS (both kinds of frame count the resolved pixels' samples, so equal totals are equal traced rays).

    python profiles/adaptive_rate.py overhead|gain [--rounds K] [--warmup W] [--plain-only] [--tree DIR] [--label NAME] [--out FILE]
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

W, H, DEPTH, SPP, STEP, SEED = 1920, 1080, 8, 64, 8, 2019
REF_SPP, REF_SEED = 2048, 77
PASSES = [(b, b + STEP) for b in range(0, SPP, STEP)]


def stats_of(ms):
    ms = np.asarray(ms, np.float64)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4), "ms_max": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["overhead", "gain"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library are measured (--plain-only: the parent's)")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--scenes", default="cornell,soup100000")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from importlib import import_module
    sys.path.insert(0, os.path.abspath(a.tree))
    gi = import_module("2019global_amd")
    S = import_module("2019global_amd.scenes")
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    lines = []

    def emit(rec):
        rec = dict({"label": a.label, "frame": [W, H], "depth": DEPTH, "spp": SPP, "pass": STEP}, **rec)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    n = W * H
    st = torch.cuda.Stream()
    rgb = torch.empty(3 * n, dtype=torch.float64, device="cuda")
    rgb8 = torch.empty(3 * n, dtype=torch.uint8, device="cuda")
    nn = torch.empty(n, dtype=torch.int32, device="cuda")
    stats = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")

    def timed(go):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        go()
        e1.record(st)
        return e0, e1

    def frames(dev, cam, light):
        kw = dict(depth=DEPTH, seed=SEED, stream=st.cuda_stream)

        def one_shot(spp=SPP, flags=0, **k):
            dev.render_device(cam, light, W, H, rgb.data_ptr(), rgb8.data_ptr(), mode=gi.MODE_X, spp=spp, flags=flags, **kw, **k)

        def progressive(flags=0):
            for p in PASSES:
                dev.render_device(cam, light, W, H, rgb.data_ptr(), rgb8.data_ptr(), mode=gi.MODE_X, spp=SPP, samples=p, flags=flags, **kw)

        def adaptive(tol, min_samples, relative=False, y_floor=0.05, flags=0, **k):
            for p in PASSES:
                dev.render_adaptive_device(cam, light, W, H, p, spp=SPP, tol=tol, min_samples=min_samples, relative=relative,
                                           y_floor=y_floor, flags=flags, d_rgb=rgb.data_ptr(), d_rgb8=rgb8.data_ptr(), d_n=nn.data_ptr(),
                                           **kw, **k)
        return one_shot, progressive, adaptive

    def rounds(cfgs):
        """cfgs {name: callable}: warm-up, then --rounds interleaved rounds; {name: [ms]}"""
        ev = {k: [] for k in cfgs}
        with torch.cuda.stream(st):
            for r in range(a.warmup + a.rounds):
                for k, go in cfgs.items():
                    e = timed(go)
                    if r >= a.warmup:
                        ev[k].append(e)
        st.synchronize()
        return {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}

    if a.what == "overhead":
        sc = S.named_scene("cornell")
        dev = gi.DeviceScene.from_scene(sc)
        cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
        one_shot, progressive, adaptive = frames(dev, cam, sc.light)
        cfgs = {"one_shot": one_shot, "progressive_8": progressive}
        if not a.plain_only:
            cfgs["adaptive_8_tol_5e-324"] = lambda: adaptive(5e-324, 2)
        ms = rounds(cfgs)
        for k, v in ms.items():
            emit(dict({"scene": "cornell", "what": "overhead", "config": k, "rounds": a.rounds}, **stats_of(v)))
        # the passes' dominant kernel (GI_FLAG_TIME) and what is left of a pass
        for k in [c for c in cfgs if c != "one_shot"]:
            per_pass, kern = [], []
            for r in range(a.rounds):
                with torch.cuda.stream(st):
                    evs = []
                    for p in PASSES:
                        if k == "progressive_8":
                            go = lambda p=p: dev.render_device(cam, sc.light, W, H, rgb.data_ptr(), rgb8.data_ptr(), mode=gi.MODE_X, spp=SPP,   # noqa: E731
                                                               samples=p, flags=gi.FLAG_TIME, depth=DEPTH, seed=SEED, stream=st.cuda_stream)
                        else:
                            go = lambda p=p: dev.render_adaptive_device(cam, sc.light, W, H, p, spp=SPP, tol=5e-324, min_samples=2,   # noqa: E731
                                                                        flags=gi.FLAG_TIME, d_rgb=rgb.data_ptr(), d_rgb8=rgb8.data_ptr(),
                                                                        depth=DEPTH, seed=SEED, stream=st.cuda_stream)
                        evs.append(timed(go))
                st.synchronize()
                kms, cnt = dev.kernel_ms()
                assert cnt == len(PASSES)
                later = [e0.elapsed_time(e1) for e0, e1 in evs[1:]]
                per_pass.append(float(np.mean(later)))
                kern.append(kms)
            other = np.array(per_pass) - np.array(kern)   # (kern averages all 8 passes, the first included: they trace alike)
            rec = {"scene": "cornell", "what": "between_the_render_kernels", "config": k, "rounds": a.rounds,
                   "pass_ms_median": round(float(np.median(per_pass)), 4), "kernel_ms_median": round(float(np.median(kern)), 4),
                   "other_ms_per_pass_median": round(float(np.median(other)), 4), "other_ms_per_pass_min": round(float(other.min()), 4),
                   "other_ms_per_pass_max": round(float(other.max()), 4)}
            if k != "progressive_8":
                act = dev.adaptive_info()["active"]   # (0 after the last pass; the passes' count: the n plane)
                adaptive(5e-324, 2)
                st.synchronize()
                listed = int((nn == SPP).sum().item())
                slots = ((W + 7) // 8) * ((H + 7) // 8) * 64
                bytes_ = listed * (24 * STEP + 48 + 48 + 4 + 4 + 4 + 24 + 3) + slots * 4
                rec.update({"active_after_last": act, "pixels_at_64": listed, "stream_bytes_per_pass": bytes_,
                            "stream_floor_ms": round(bytes_ / COPY_BYTES_PER_S * 1e3, 4),
                            "times_the_floor": round(float(np.median(other)) / (bytes_ / COPY_BYTES_PER_S * 1e3), 2)})
            emit(rec)
        dev.close()
    else:
        for name in a.scenes.split(","):
            sc = S.named_scene(name)
            dev = gi.DeviceScene.from_scene(sc)
            cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
            one_shot, progressive, adaptive = frames(dev, cam, sc.light)
            with torch.cuda.stream(st):
                dev.render_device(cam, sc.light, W, H, rgb.data_ptr(), mode=gi.MODE_X, spp=REF_SPP, depth=DEPTH, seed=REF_SEED,
                                  stream=st.cuda_stream)
            st.synchronize()
            truth = rgb.clone()

            def measure(go):
                stats.zero_()
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    go(stats_ptr=stats.data_ptr())
                st.synchronize()
                rays = int(stats[gi.STAT_RAYS].item())
                mse = float(((rgb - truth) ** 2).mean().item())
                return rays, mse

            plain_done = {}

            def plain(k, why):
                if k not in plain_done:
                    pgo = lambda **kk: one_shot(spp=k, **kk)   # noqa: E731
                    prays, pmse = measure(pgo)
                    pms = rounds({"plain": pgo})["plain"]
                    plain_done[k] = dict({"scene": name, "what": "gain", "config": "plain", "spp_plain": k, "mean_n": float(k),
                                          "rays": prays, "mse": pmse, "rounds": a.rounds}, **stats_of(pms))
                    emit(dict(plain_done[k], chosen_by=why))
                return plain_done[k]
            # GI_STAT_RAYS grows linearly with a plain frame's spp (the resolved pixels' samples are counted in both kinds
            # of frame, in every pass): the plain frame of equal rays is the one of rays / rays_per_spp samples
            rays_per_spp = (plain(16, "slope")["rays"] - plain(8, "slope")["rays"]) / 8.0
            for relative in (False, True):
                for tol in (0.005, 0.01, 0.02, 0.04, 0.08):
                    go = lambda **k: adaptive(tol, 8, relative=relative, **k)   # noqa: E731
                    rays, mse = measure(go)
                    mean_n = float(nn.double().mean().item())
                    ms = rounds({"adaptive": go})["adaptive"]
                    k_n = max(2, min(SPP, int(round(mean_n))))
                    k_rays = max(2, min(SPP, int(round(rays / rays_per_spp))))
                    emit(dict({"scene": name, "what": "gain", "config": "adaptive", "relative": relative, "tol": tol, "y_floor": 0.05,
                               "min_samples": 8, "mean_n": round(mean_n, 3), "rays": rays, "mse": mse, "rounds": a.rounds,
                               "plain_spp_nearest_mean_n": k_n, "plain_spp_of_equal_rays": k_rays}, **stats_of(ms)))
                    plain(k_n, "mean n")
                    plain(k_rays, "equal rays")
            dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
