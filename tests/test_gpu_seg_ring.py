"""GPU checks of k_seg's per-wave ring of prepared primary rays (gi_wf.hip k_seg<..., RING>; DESIGN.md
§5): all 64 lanes of a wave generate a batch of 64 units at once and park the primary rays that hit the
root box in LDS, and lanes whose path has ended pop one.  Frames and ray counts must not change: against
the direct path (GI_SEG_RING=0, read once per process: child processes), against the CPU oracle, and a
progressive frame against the one-shot frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_util as U

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()

SEED = 2019
FAR_BACK = 2000.0   # the far triangle's camera: the scene camera's distance from its look-at point x this
STATS = ("STAT_RAYS", "STAT_X_RESOLVED", "STAT_PIXELS", "STAT_NODES", "STAT_PRIMS")

# name: (scene, w, h, spp, depth, options, ring expected, oracle).  The smallest shapes at which the ring
# can go wrong.  scene: a named scene, or "x:<function>" of tests/x_scenes.py.  options: shard, passes,
# env (the processes' environment); focal / back: the scene's camera with its focal length scaled (a
# small frame sees only the middle of the view: a shorter focal length brings the scene's outline into
# it) or moved back along its view line by that factor; gen: the case counts the samples k_seg resolves
# where it generates them (below) and must find some; runs128: the launch must be large enough for
# 128-unit runs.
# `ring expected` is what gi_scene_seg_ring must say in a process without GI_SEG_RING=0, from the LDS
# arithmetic of DESIGN.md §5 on a CU's 163,840 B:
#   the Cornell box, flat kernels: 13,600 B of records + 128 + 16,384 of path slots + 10,240 of ring =
#     40,352 B, four workgroups 161,408 B: fits, on.  Walking the tree (GI_X_FLAT=0) stages the 768 B of
#     wide nodes too: 41,120 B, four workgroups 164,480 B: a workgroup fewer per CU, off.
#   `main` (spheres: 3 waves per SIMD; a few hundred bytes of records), the one triangle, the three-quad
#     corner (six triangles: well under the 14,208 B of records that leave the ring room at four
#     workgroups) and soup1000 (HBM-resident: level stack 16,384 + slots 16,384 + ring 10,240 = 43,008 B,
#     three workgroups 129,024 B): on.
CASES = {
    # at most one partial batch; the one-sample store path (the pixel, not a per-sample row)
    "cornell_8x8_1spp": ("cornell", 8, 8, 1, 8, {}, True, False),
    # units no multiple of 64; a batch spans many work-list entries
    "cornell_24x16_3spp": ("cornell", 24, 16, 3, 8, {}, True, True),
    # depth 1: every lane ends every segment, each iteration pops 64 and the ring drains exactly
    "cornell_64x48_5spp_d1": ("cornell", 64, 48, 5, 1, {}, True, True),
    # depth 8: partial pops that leave entries for the next iteration
    "cornell_64x48_5spp_d8": ("cornell", 64, 48, 5, 8, {}, True, True),
    # the main.cpp scene: the 3-wave kernels with sphere primitives, short paths (every lane pops nearly
    # every iteration).  With the scene's own camera a frame this small shows no background (the next
    # three cases do)
    "main_96x64_4spp": ("main", 96, 64, 4, 3, {}, True, False),
    # ... with a quarter and a tenth of the focal length: the scene's outline crosses the frame, listed
    # pixels on it lose some of their samples to the root-box pretest inside a batch (the hit ballot is
    # sparse: entries compacted by rank, zero rows stored from the batch); at a tenth the frame is
    # background-heavy
    "main_96x64_4spp_f025": ("main", 96, 64, 4, 3, {"focal": 0.25, "gen": True}, True, False),
    "main_96x64_4spp_f01": ("main", 96, 64, 4, 3, {"focal": 0.1, "gen": True}, True, False),
    # a launch of more than 2 x 64 x 8 units per resident wave: k_seg takes 128-unit runs, two batches
    # each (and its outline pixels lose samples).  Against GI_SEG_RING=0 only
    "main_640x400_24spp_runs128": ("main", 640, 400, 24, 2, {"gen": True, "runs128": True}, True, False),
    # one triangle from so far that its box is a small fraction of a pixel: the few listed pixels lose
    # nearly all their samples -- fewer hits than batches, so some batches push no entry at all, a burst
    # retries across them, and a wave's loop passes through "no lane live, not done"
    "one_triangle_far_16x16_256spp": ("x:one_triangle", 16, 16, 256, 3, {"back": FAR_BACK, "gen": True}, True, False),
    # an HBM-resident k_seg variant: the ring beside the level stack
    "soup1000_48x32_2spp": ("soup1000", 48, 32, 2, 4, {}, True, False),
    # an LDS-resident scene that walks its tree (octree-shaped, no flat table) and keeps the ring:
    # k_seg<LDS, FLAT = false, RING = true>
    "corner3_octree_48x32_3spp": ("x:corner3_octree", 48, 32, 3, 4, {}, True, False),
    # packed tiles of one shard of three
    "cornell_40x24_shard": ("cornell", 40, 24, 2, 8, {"shard": (3, 1)}, True, False),
    # progressive passes [0, 2) and [2, 6); compared with the one-shot frame below as well
    "cornell_16x16_passes": ("cornell", 16, 16, 6, 8, {"passes": ((0, 2), (2, 6))}, True, False),
    "cornell_16x16_oneshot": ("cornell", 16, 16, 6, 8, {}, True, False),
    "cornell_mirror_24x16_4spp": ("cornell_mirror", 24, 16, 4, 8, {}, True, False),
    # the Cornell box walking its tree (its processes run with GI_X_FLAT=0), which stages its nodes and
    # so has no room for the ring: this case checks the host's rule (gi_scene_seg_ring says off, and the
    # launch then runs the direct path) -- its frame comparison is direct path against direct path
    "cornell_24x16_tree": ("cornell", 24, 16, 3, 8, {"env": {"GI_X_FLAT": "0"}}, False, False),
}
FLAT_CASES = [n for n, c in CASES.items() if "env" not in c[5]]
TREE_CASES = [n for n, c in CASES.items() if "env" in c[5]]


def _scene(scene):
    """(scene, the environment its DeviceScene is built under)"""
    if scene.startswith("x:"):
        import x_scenes
        return getattr(x_scenes, scene[2:])()
    return S.named_scene(scene), {}


def _device_scene(sc, env):
    from x_scenes import with_env
    return with_env(env, lambda: gi.DeviceScene.from_scene(sc))


def _stats_render(torch, d, cam, sc, w, h, n, spp, depth, samples, kw, st=None, bufs=None):
    st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda") if st is None else st
    buf, buf8 = bufs or (torch.zeros(n * 3, dtype=torch.float64, device="cuda"), torch.zeros(n * 3, dtype=torch.uint8, device="cuda"))
    d.render_device(cam, sc.light, w, h, buf.data_ptr(), buf8.data_ptr(), mode=gi.MODE_X, spp=spp, depth=depth,
                    seed=SEED, stats_ptr=st.data_ptr(), samples=samples, **kw)
    torch.cuda.synchronize()
    return st, buf, buf8


def render_case(torch, name):
    """One case on the device, with statistics: fp64 radiance, RGB888, the STATS totals, what
    gi_scene_seg_ring and gi_scene_x_form say.  gen cases also: the units k_seg was given and the samples
    it resolved where it generated them.  The statistics hold only sums with the classify pass's (a
    background pixel adds its spp to STAT_X_RESOLVED and 1 to STAT_PIXELS), so the background pixels are
    counted apart: in a progressive pass that begins after sample 0, k_seg adds nothing to STAT_PIXELS (it
    counts a pixel at its sample 0), so that pass's STAT_PIXELS is the classify pass's count."""
    scene, w, h, spp, depth, opt, _, _ = CASES[name]
    sc, env = _scene(scene)
    d = _device_scene(sc, env)
    back = opt.get("back", 1.0)
    pos = tuple(l + back * (p - l) for p, l in zip(sc.cam_pos, sc.cam_look))
    cam = gi.Camera(pos, sc.cam_look, sc.focal * opt.get("focal", 1.0))
    n = w * h
    kw = {}
    if "shard" in opt:
        n = gi.shard_tiles(w, h, opt["shard"][0]) * gi.TILE * gi.TILE
        kw = dict(shard_count=opt["shard"][0], shard_index=opt["shard"][1])
    st = bufs = None
    for samples in opt.get("passes", (None,)):
        st, *bufs = _stats_render(torch, d, cam, sc, w, h, n, spp, depth, samples, kw, st, bufs)
    stats = st.cpu().numpy()
    gen = units = -1
    if opt.get("gen"):
        d2 = _device_scene(sc, env)
        _stats_render(torch, d2, cam, sc, w, h, n, spp, depth, (0, 1), kw)
        st2 = _stats_render(torch, d2, cam, sc, w, h, n, spp, depth, (1, 2), kw)[0].cpu().numpy()
        n_bg = int(st2[gi.STAT_PIXELS])
        units = (w * h - n_bg) * spp
        gen = int(stats[gi.STAT_X_RESOLVED]) - n_bg * spp
    return dict(rgb=bufs[0].cpu().numpy().view(np.int64), rgb8=bufs[1].cpu().numpy(),
                stats=np.array([int(stats[getattr(gi, s)]) for s in STATS], np.int64),
                ring=np.array([int(d.seg_ring(spp=spp, depth=depth))]),
                seg=np.array([int(d.x_form(spp=spp, depth=depth) == "k_seg")]),
                gen=np.array([gen, units], np.int64), cus=np.array([torch.cuda.get_device_properties(0).multi_processor_count]))


def render_cases(names, out):
    """(Also the child processes' entry point.)"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    res = {}
    for name in names:
        for k, v in render_case(torch, name).items():
            res[name + "/" + k] = v
    if out:
        np.savez(out, **res)
    return res


def _child(names, out, env):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_seg_ring as T; "
            "T.render_cases(%r, %r)") % (U.ROOT, os.path.join(U.ROOT, "tests"), names, out)
    return subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **env))


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """Every case once with the ring (this process; the GI_X_FLAT=0 case in a child) and once with
    GI_SEG_RING=0 (children).  The three children run side by side; none outlives the fixture."""
    tmp = tmp_path_factory.mktemp("seg_ring")
    jobs = [(FLAT_CASES, str(tmp / "direct.npz"), {"GI_SEG_RING": "0"}),
            (TREE_CASES, str(tmp / "direct_tree.npz"), {"GI_SEG_RING": "0", "GI_X_FLAT": "0"}),
            (TREE_CASES, str(tmp / "ring_tree.npz"), {"GI_X_FLAT": "0"})]
    procs = []
    try:
        for j in jobs:
            procs.append(_child(*j))
        ring = render_cases(FLAT_CASES, None)
        codes = [p.wait(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    assert codes == [0, 0, 0]
    direct = dict(np.load(jobs[0][1]).items())
    direct.update(np.load(jobs[1][1]).items())
    ring.update(np.load(jobs[2][1]).items())
    return ring, direct


@pytest.mark.parametrize("name", sorted(CASES))
def test_ring_equals_direct_path(frames, name):
    """fp64 radiance bit for bit, the same RGB888, and the same totals of rays, resolved samples, pixels,
    node visits and primitive tests with the ring and with GI_SEG_RING=0; k_seg runs in both, and
    gi_scene_seg_ring says what the LDS arithmetic says (CASES) and 0 under GI_SEG_RING=0.  (Where the
    ring is expected off -- the GI_X_FLAT=0 case -- both sides run the direct path: that case checks the
    host's rule, not the ring.)"""
    ring, direct = frames
    assert ring[name + "/seg"][0] == 1 and direct[name + "/seg"][0] == 1
    assert bool(ring[name + "/ring"][0]) == CASES[name][6]
    assert direct[name + "/ring"][0] == 0
    assert (ring[name + "/rgb"] == direct[name + "/rgb"]).all()
    assert (ring[name + "/rgb8"] == direct[name + "/rgb8"]).all()
    assert (ring[name + "/rgb"].view(np.float64) > 0).any()
    got, want = ring[name + "/stats"], direct[name + "/stats"]
    print(name, dict(zip(STATS, got.tolist())), dict(zip(STATS, want.tolist())), "gen, units", ring[name + "/gen"].tolist())
    assert (got == want).all(), dict(zip(STATS, zip(got.tolist(), want.tolist())))
    assert got[0] > 0 and got[2] > 0


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n][5].get("gen")])
def test_ring_resolves_root_box_misses_in_batches(frames, name):
    """The cases whose frame shows the scene's outline: of the units k_seg is given, some -- not none, not
    all -- miss the root box and are resolved where they are generated, inside a batch whose hit ballot is
    then sparse; the same number with the ring and with GI_SEG_RING=0 (and the frames equal: the test
    above).  The far triangle: all but fewer than one per batch, so that some batches push no entry.  The large launch:
    its units exceed 2 x 64 x 8 per wave of the most k_seg waves the device can hold (4 workgroups of 4
    waves per CU), the size from which k_seg's runs are 128 units."""
    ring, direct = frames
    gen, units = (int(v) for v in ring[name + "/gen"])
    assert (ring[name + "/gen"] == direct[name + "/gen"]).all()
    assert 0 < gen < units, (gen, units)
    if name.startswith("one_triangle_far"):   # (a launch this small takes 64-unit runs: units / 64 batches)
        assert units - gen < units // 64, (gen, units)   # fewer hits than batches: some batch is empty
    if CASES[name][5].get("runs128"):
        assert units >= 2 * 64 * 8 * 16 * int(ring[name + "/cus"][0]), units


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n][7]])
def test_ring_frame_bit_exact_to_oracle(frames, name):
    """The 24 x 16 and 64 x 48 Cornell frames rendered with the ring equal the CPU oracle's bit for bit."""
    scene, w, h, spp, depth = CASES[name][:5]
    o = U.oracle_render(_scene(scene)[0].to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=SEED)
    same = U.bits_equal(frames[0][name + "/rgb"].view(np.float64).reshape(-1, 3), o["rgb"]).all(1)
    assert same.all(), f"{name}: {int((~same).sum())} of {same.size} pixels differ"


def test_ring_progressive_passes_equal_one_shot(frames):
    """Passes [0, 2) and [2, 6) (the second continues the work list; its units start at sample 2) give
    the 6-sample frame of one launch, with the ring and without."""
    for res in frames:
        assert (res["cornell_16x16_passes/rgb"] == res["cornell_16x16_oneshot/rgb"]).all()
        assert (res["cornell_16x16_passes/rgb8"] == res["cornell_16x16_oneshot/rgb8"]).all()
