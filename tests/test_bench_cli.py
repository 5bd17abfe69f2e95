"""bench.py's command line: a plain run prints the headline line and nothing that takes a run of its own
(those sit behind --full), and --dump-outputs writes the last timed frame -- the same pixels from run to
run, equal to a render of the same workload through the C-ABI."""
import json
import sys

import numpy as np
import pytest

import oracle_util as U

sys.path.insert(0, U.ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SIDE = ("host_path", "ms_per_frame_with_d2h", "cpu_baseline", "reference_cpu", "frame_check")


def test_dump_sample_is_fixed_sorted_and_within_budget():
    assert bench.dump_pixels(512 * 512, "rgb", 8) is None          # a small frame is dumped whole
    assert bench.dump_pixels(1920 * 1080, "rgb", 8) is None        # the default workload's radiance too
    total = 0
    for name, itemsize in (("rgb", 8), ("rgb8", 4)):
        n = 3840 * 2160
        a, b = bench.dump_pixels(n, name, itemsize), bench.dump_pixels(n, name, itemsize)
        assert (a == b).all() and (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < n
        assert len(a) * 3 * itemsize <= bench.DUMP_BUDGET[name]
        total += bench.DUMP_BUDGET[name]
    assert total + 2 * 128 <= 64_000_000                            # both files with their .npy headers


def _run(capsys, *argv):
    bench.main(["--gpus", "1", "--workload", "C2", *argv])
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_frame(tmp_path, capsys):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _run(capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(a))
    assert all(k in d for k in HEADLINE) and not any(k in d for k in SIDE)
    assert d["steps"] == 3 and d["unit"] == "Mray/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = traced rays per second over the timed steps, ms_per_step = one of those steps
    assert d["value"] == pytest.approx(d["config"]["rays_traced_per_frame"] / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    _run(capsys, "--steps", "2", "--warmup", "0", "--dump-outputs", str(b))
    scene, w, h, mode, spp, depth, _ = bench.WORKLOADS["C2"]
    gi, sc = U.pkg(), bench.make_scene(scene)
    rgb, rgb8 = gi.DeviceScene.from_scene(sc).render(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, w, h,
                                                     mode=mode, spp=spp, depth=depth, seed=2019)
    for out in (a, b):
        got, got8 = np.load(out / "rgb.npy"), np.load(out / "rgb8.npy")
        assert got.dtype == np.float64 and got.shape == (w * h, 3) and got8.dtype == np.float32
        assert U.bits_equal(got, rgb.reshape(-1, 3)).all()
        assert (got8 == rgb8.reshape(-1, 3)).all()


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements(capsys):
    d = _run(capsys, "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert all(k in d for k in HEADLINE)
    assert d["host_path"]["ms_per_frame"]["rgb8"] == d["ms_per_frame_with_d2h"] > 0
    assert "cpu_baseline" not in d
