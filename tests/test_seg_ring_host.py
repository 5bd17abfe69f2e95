"""k_seg's unit accounting on the CPU: 2019global_amd/csrc/gi_seg_ring.h SegUnits -- the functions the
kernel calls to hand out its units a batch at a time and to fill and drain its per-wave ring of prepared
primary rays -- driven by tests/cpp/seg_ring_check.cpp for simulated waves that share one counter."""
import os
import subprocess

import oracle_util as U

CSRC = os.path.join(U.ROOT, "2019global_amd", "csrc")
SRC = os.path.join(U.ROOT, "tests", "cpp", "seg_ring_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, "-I" + os.path.join(U.ROOT, "include")]
TOTALS = [0, 1, 63, 64, 65, 127, 128, 129, 64 * 1024 + 1]


def _check(out):
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout[-3000:]
    assert lines[-1] == "failures 0", out.stdout[-3000:]
    for total in TOTALS:
        for run in (64, 128):
            assert f"total {total} run {run}: failures 0" in lines, (total, run)


def test_seg_ring_accounting(tmp_path):
    """Totals of 0, 1, 63, 64, 65, 127, 128, 129 and 64 k + 1 units in runs of 64 and 128, 1 / 3 / 16 waves
    on one counter, seeded random need masks (every lane ends every segment, a fifth, few) and miss masks
    (none, a quarter, most, all): every unit generated exactly once, every hit popped exactly once by a
    lane that needed one, never more than 64 entries in a ring, every wave ends with an empty ring."""
    exe = str(tmp_path / "seg_ring")
    subprocess.run(["g++", "-O2", *FLAGS, "-o", exe, SRC], check=True)
    out = subprocess.run([exe, "4"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    _check(out)


def test_seg_ring_accounting_under_sanitizers(tmp_path):
    """The same stand-alone program (host code only) built with AddressSanitizer and
    UndefinedBehaviorSanitizer: no report, 0 failures."""
    exe = str(tmp_path / "seg_ring_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", *FLAGS, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, "1"], capture_output=True, text=True, env=env, timeout=300)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    _check(out)
