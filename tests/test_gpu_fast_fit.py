"""bmfr_config.fast_fit = 1: the Householder trailing update (bmfr.cl:606-655)
as one fused multiply-add per element on the block-wide factor
2 dot / |u|^2 instead of upstream's three roundings, and (half tmp_data) the
wave-wide sums / minima / maxima as butterflies instead of upstream's
association (bmfr.cl:25-85), the step-0 noise added in f32 (bmfr.cl:173-182),
the pivot's square root and reciprocal and the feature scaling at hardware
precision -- no longer bit-exact,
so it is held to north_star's floating-point bar instead: the frame output
within 1e-4 relative L2 of the reference kernels (oracle/_ref, strict and
default builds) on the same inputs, at the BASELINE sizes (half and f32
tmp_data, B = 13 and 16) over all 16 block-grid offsets and over a whole
60-frame sequence (the error does not
build up through the temporal accumulation).  The fused update changes only
the fit's arithmetic, so everything else is checked bit for bit as for the
exact path: the frame APIs (per-frame one launch, profiled two launches,
whole sequence, tiled) agree with each other, and the temporal state the fit
does not touch (noisy accumulation, spp, reprojected positions) equals the
reference's."""
from __future__ import annotations

import pytest
import torch

import bmfr_amd
import ref_run
from parity_harness import fused_state, rel_l2, same_bits
from ref_configs import FULL_REF_CONFIGS
from seq_util import PLANES, TOL

pytestmark = pytest.mark.gpu


def frames_of(W, H, n, **kw):
    cfg = bmfr_amd.BmfrConfig(image_width=W, image_height=H, fast_fit=1, **kw)
    frames = [bmfr_amd.synth_frame_device(W, H, f) for f in range(n)]
    if kw.get("input_half"):  # half3 input planes (the f32 render rounded to nearest)
        frames = [{k: (v.half() if k in PLANES else v) for k, v in fr.items()} for fr in frames]
    return cfg, frames


def run_frames(cfg, frames, profiled=False):
    W, H = cfg.image_width, cfg.image_height
    den = bmfr_amd.Denoiser(cfg)
    if profiled:  # per-kernel events: K1 (k_fused_cols<..., FAST>) and K2 as two launches
        den.set_profiling(True, capacity=len(frames), stride=1)
    out = []
    for f, fr in enumerate(frames):
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f)
        out.append(fused_state(den, W * H, host=False))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("W,H,n,kw", [(200, 136, 20, {}), (1920, 1080, 6, {}),
                                      (256, 144, 6, {"scaled": bmfr_amd.SCALED_THIRD_ORDER}),
                                      (200, 136, 8, {"use_half_precision_in_tmp_data": 0}),
                                      (256, 144, 6, {"use_half_precision_in_tmp_data": 0,
                                                     "scaled": bmfr_amd.SCALED_THIRD_ORDER}),
                                      (256, 144, 6, {"use_half_precision_in_tmp_data": 0, "input_half": 1,
                                                     "scaled": bmfr_amd.SCALED_THIRD_ORDER})])
def test_fast_fit_frame_apis_agree(W, H, n, kw, gpu):
    """One-launch frames == profiled two-launch frames == one
    bmfr_process_sequence call, bit for bit, and the fast fit really differs
    from the exact one."""
    cfg, frames = frames_of(W, H, n, **kw)
    one, two = run_frames(cfg, frames), run_frames(cfg, frames, profiled=True)
    den = bmfr_amd.Denoiser(cfg)
    cams = [(bmfr_amd.synth_camera(W, H, max(f - 1, 0))[0], bmfr_amd.synth_camera(W, H, f)[1]) for f in range(n)]
    outs = [torch.empty(3 * W * H, device="cuda") for _ in range(n)]
    den.process_sequence(frames, cams, 0, outputs=outs)
    torch.cuda.synchronize()
    for f in range(n):
        for k in one[f]:
            assert same_bits(one[f][k], two[f][k]), f"frame {f} {k}: one launch != two launches"
        assert same_bits(one[f]["result"], outs[f]), f"frame {f}: per-frame != sequence"
    exact = run_frames(bmfr_amd.BmfrConfig(image_width=W, image_height=H, **kw), frames)
    assert not same_bits(exact[-1]["result"], one[-1]["result"])
    assert rel_l2(one[-1]["result"], exact[-1]["result"]) < TOL


# (reference build, frames): every block-grid offset at 1080p / 4K, B = 16, 60-frame sequences (720p, 4K and
# BASELINE config 2's 1080p)
CASES = [("f1920x1080_h13", 17), ("f3840x2160_h13", 17), ("f3840x2160_h16", 17), ("f3840x2160_f13", 17),
         ("f1280x720_h13", 60), ("f3840x2160_h13", 60), ("f1920x1080_h13", 60)]


@pytest.mark.parametrize("name,n", CASES)
def test_fast_fit_within_tolerance_of_reference(name, n, gpu, parity_log):
    rc = FULL_REF_CONFIGS[name]
    if not ref_run.available(rc.name):
        pytest.fail(f"reference build {rc.name} missing (oracle/build_ref.py)")
    W, H = rc.width, rc.height
    cfg = bmfr_amd.BmfrConfig(image_width=W, image_height=H, scaled=rc.scaled, library_powr=1, fast_fit=1,
                              use_half_precision_in_tmp_data=rc.half_tmp)
    den = bmfr_amd.Denoiser(cfg)
    refs = {m: ref_run.RefLoop(rc, m) for m in ("strict", "default") if ref_run.available(rc.name, m)}
    worst = {m: 0.0 for m in refs}
    per_frame = {m: [] for m in refs}  # error growth along the temporal accumulation
    for f in range(n):
        fr = bmfr_amd.synth_frame_device(W, H, f)
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f)
        got = fused_state(den, W * H, host=False)
        for m, rl in refs.items():
            rec = {}
            rl.upload(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"])
            rl.run_stages(vp, jit, f, record=rec)
            rl.swap()
            e = rel_l2(got["result"], rec["result"])
            worst[m] = max(worst[m], e)
            per_frame[m].append(float(f"{e:.3e}"))
            assert e <= TOL, (name, f, m, e)
            if m == "strict":  # the fit does not feed these
                for k in ("noisy", "spp", "prev_pixel"):
                    assert same_bits(got[k], rec[k]), (name, f, k)
    parity_log(f"fast_fit_{name}" + ("" if n == 17 else f"_{n}frames"),
               {"frames": n, "worst_rel_l2": worst, "per_frame_rel_l2": per_frame})
    print(f"{name}: fast_fit worst output rel-L2 {worst}")


def test_bench_configuration_within_tolerance_of_reference(gpu, parity_log):
    """The exact configuration bench.py's headline times -- 3840x2160, B = 13,
    half tmp_data, fast_fit, the correctly rounded powr (library_powr = 0) --
    per frame against the reference's strict build, 17 frames (every
    block-grid offset): output within 1e-4 relative L2 (the powr's last-bit
    differences add ~1e-7 to the fit's ~1.2e-5), temporal state the fit does
    not feed bit for bit."""
    rc = FULL_REF_CONFIGS["f3840x2160_h13"]
    if not ref_run.available(rc.name):
        pytest.fail(f"reference build {rc.name} missing (oracle/build_ref.py)")
    W, H = rc.width, rc.height
    den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, fast_fit=1))
    ref = ref_run.RefLoop(rc, "strict")
    worst = 0.0
    for f in range(rc.frames):
        fr = bmfr_amd.synth_frame_device(W, H, f)
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f)
        got = fused_state(den, W * H, host=False)
        rec = {}
        ref.upload(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"])
        ref.run_stages(vp, jit, f, record=rec)
        ref.swap()
        e = rel_l2(got["result"], rec["result"])
        worst = max(worst, e)
        assert e <= TOL, (f, e)
        for k in ("noisy", "spp", "prev_pixel"):
            assert same_bits(got[k], rec[k]), (f, k)
    parity_log("fast_fit_bench_configuration_f3840x2160_h13", {"frames": rc.frames, "worst_rel_l2_vs_strict": worst})
    print(f"bench configuration: worst output rel-L2 vs the strict reference {worst:.3g}")


def test_cfg5_timed_configuration_within_tolerance_of_reference(gpu, parity_log):
    """BASELINE config 5 exactly as bench.py times it (ms_per_frame_cfg5):
    3840x2160, half input planes, B = 16 (3rd-order positions), half
    tmp_data, fast_fit, the correctly rounded powr -- per frame against the
    reference kernels run on the same planes widened to f32 (what the half
    path reads), 17 frames (every block-grid offset): output within 1e-4
    relative L2 of the strict and the default build, the temporal state the
    fit does not feed bit for bit (strict)."""
    rc = FULL_REF_CONFIGS["f3840x2160_h16"]
    if not ref_run.available(rc.name):
        pytest.fail(f"reference build {rc.name} missing (oracle/build_ref.py)")
    W, H = rc.width, rc.height
    den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, scaled=rc.scaled, fast_fit=1,
                                                input_half=1))
    refs = {m: ref_run.RefLoop(rc, m) for m in ("strict", "default") if ref_run.available(rc.name, m)}
    worst = {m: 0.0 for m in refs}
    for f in range(rc.frames):
        fr = bmfr_amd.synth_frame_device(W, H, f, seed=rc.seed)
        h = {k: fr[k].half() for k in PLANES}
        w = {k: v.float() for k, v in h.items()}
        del fr
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        den.process_frame(h["noisy"], h["normals"], h["positions"], h["albedo"], vp, jit, f)
        got = fused_state(den, W * H, host=False)
        for m, rl in refs.items():
            rec = {}
            rl.upload(w["noisy"], w["normals"], w["positions"], w["albedo"])
            rl.run_stages(vp, jit, f, record=rec)
            rl.swap()
            e = rel_l2(got["result"], rec["result"])
            worst[m] = max(worst[m], e)
            assert e <= TOL, (f, m, e)
            if m == "strict":
                for k in ("noisy", "spp", "prev_pixel"):
                    assert same_bits(got[k], rec[k]), (f, k)
    parity_log("fast_fit_cfg5_timed_f3840x2160_h16_in16", {"frames": rc.frames, "worst_rel_l2": worst})
    print(f"config 5 timed configuration: worst output rel-L2 {worst}")


def test_fast_fit_tiled_matches_untiled(gpu):
    """The fit is per block: a 2x2 tiling with fast_fit equals the untiled
    fast_fit frames bit for bit (halo exchanged by the loopback transport,
    as tests/test_gpu_tiled.py does for the exact path)."""
    from bmfr_amd.tiling import HipCopier, LoopbackTransport, TileGrid, state_planes
    W, H, n, halo = 320, 256, 6, 40
    cfg, frames = frames_of(W, H, n)
    full = run_frames(cfg, frames)
    grid = TileGrid(W, H, 2, 2, halo=halo)
    tiles = [bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, fast_fit=1, tile=grid.tile(r),
                                                   tile_halo=halo)) for r in range(grid.ranks)]
    loop, copier = LoopbackTransport(grid), HipCopier()
    prev = [None] * grid.ranks
    for f in range(n):
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        inps = [bmfr_amd.synth_region_device(W, H, d.region, f) for d in tiles]
        if f > 0:
            loop.exchange_all([state_planes(d) for d in tiles], copier)
        for r, d in enumerate(tiles):
            i = inps[r]
            d.process_frame(i["noisy"], i["normals"], i["positions"], i["albedo"], vp, jit, f,
                            prev_normals=prev[r]["normals"] if prev[r] else None,
                            prev_positions=prev[r]["positions"] if prev[r] else None)
        prev = inps
        torch.cuda.synchronize()
        want = full[f]["result"].view(H, W, 3)
        for r, d in enumerate(tiles):
            x0, y0, w, h = d.region
            got = d.copy_output(torch.empty(w * h * 3, device="cuda")).view(h, w, 3)
            tx, ty, tw, th = grid.tile(r)
            a = got[ty - y0:ty - y0 + th, tx - x0:tx - x0 + tw].contiguous()
            assert same_bits(a, want[ty:ty + th, tx:tx + tw].contiguous()), f"frame {f} tile {r}"


def test_fast_fit_without_sched_barrier(gpu, tmp_path):
    """Round 3 found the fast column update wrong (5.6e-3 rel-L2) once its
    scheduling barrier was removed: the inline-asm pivot-row FMA read a v_dot2
    result two instructions later, where gfx950 needs three wait states the
    compiler inserts only for instructions it can see (tools/isa_hazards.py).
    The FMA is compiler-visible now, so the barrier is a register knob only:
    the build without it (libbmfr_fastnosb.so, -DBMFR_FAST_SCHED_BARRIER=0,
    run in a child process) must give the default build's frames bit for bit
    -- a schedule never changes an IEEE result -- and stay within north_star's
    1e-4 of the exact path."""
    import os
    import subprocess
    import sys

    import numpy as np
    W, H, n = 200, 136, 20
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "bmfr_amd", "libbmfr_fastnosb.so")):
        pytest.fail("libbmfr_fastnosb.so missing (__graft_entry__.build())")
    out = tmp_path / "nosb.npy"
    env = dict(os.environ, BMFR_LIB="fastnosb")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "variant_frames.py"), str(W), str(H), str(n), "1",
                        str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "BMFR_FAST_SCHED_BARRIER=0" in r.stdout, r.stdout
    nosb = torch.from_numpy(np.load(out))
    cfg, frames = frames_of(W, H, n)
    fast = run_frames(cfg, frames)
    exact = run_frames(bmfr_amd.BmfrConfig(image_width=W, image_height=H), frames)
    for f in range(n):
        got = fast[f]["result"].cpu()
        assert same_bits(nosb[f], got), f"frame {f}: barrier-free build differs from the default build"
        assert rel_l2(nosb[f], exact[f]["result"].cpu()) < TOL
