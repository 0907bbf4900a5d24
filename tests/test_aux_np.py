"""tests/aux_np.py on the CPU: AuxOracleLoop -- the CPU oracle composed into
the frame loop of a feature list that names caller-supplied planes
(BMFR_FEATURE_AUX0..3) -- is pinned to pyoracle.OracleLoop itself.  Fed planes
that hold a named monomial's f32 values it must equal the oracle run with the
named codes, byte for byte, on every recorded buffer.  And the planes the GPU
content test (tests/test_gpu_aux_features.py) feeds it -- cross terms, albedo
luminance, an object-id step plane -- each change the output: otherwise that
test would show nothing."""
from __future__ import annotations

import numpy as np
import pytest

import aux_np
import pyoracle
from aux_np import AUX0
from ref_configs import REF_CONFIGS
from seq_util import ALL_KEYS, compare_exact, rel_l2, run_loop

FRAMES = 4

# configuration -> ({position in not_scaled + scaled: plane index}, plane names)
MONOMIAL = {
    # NS = 1, FS = 3, half: px and pz as planes, named out of order
    "s96x64_h7": ({1: 1, 3: 0}, ("pz", "px")),
    # NS = 2, FS = 7, half: nz and the three cubes
    "s80x64_h12": ({1: 2, 2: 0, 3: 1, 4: 3}, ("px3", "py3", "nz", "pz3")),
    # NS = 4, FS = 6, f32: nx not scaled, px^2 and py scaled
    "s128x80_f13": ({1: 0, 7: 1, 5: 2}, ("nx", "px2", "py")),
}


@pytest.mark.parametrize("name", list(MONOMIAL))
def test_monomial_planes_equal_named_codes(name):
    rc = REF_CONFIGS[name]
    subs, names = MONOMIAL[name]
    codes, was = aux_np.substitute(rc.not_scaled + rc.scaled, subs)
    for k, code in was.items():
        assert aux_np.CODE_OF[names[k]] == code, (k, names[k], code)
    ns = len(rc.not_scaled)
    loop = aux_np.AuxOracleLoop(rc.width, rc.height, codes[:ns], codes[ns:], rc.half_tmp, names)
    got = run_loop(loop, rc, FRAMES)
    cfg = pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp)
    want = run_loop(pyoracle.OracleLoop(cfg), rc, FRAMES)
    compare_exact(got, want, ALL_KEYS, f"AuxOracleLoop vs OracleLoop[{name}]")


def test_item_pixels_match_the_oracle_tmp_data():
    """The helper's work-item -> pixel map, against the oracle's own tmp_data:
    the px column (code 4) of accumulate_noisy_data holds positions.x of the
    pixel the helper names, for a frame with a non-trivial block offset."""
    rc = REF_CONFIGS["s96x64_f10"]
    cfg = pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp)
    recs = run_loop(pyoracle.OracleLoop(cfg), rc, 3)
    loop = aux_np.AuxOracleLoop(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp, ())
    col = (rc.not_scaled + rc.scaled).index(4)
    from seq_util import frame_inputs
    for f in (1, 2):
        px = np.asarray(frame_inputs(rc, f)["positions"], np.float32).reshape(-1, 3)[:, 0]
        t = recs[f]["tmp_noisy"].reshape(loop.mh // 32, loop.mw // 32, loop.B, 32, 32)
        assert t[:, :, col].tobytes() == px[loop.item_pixels(f)].tobytes(), f


@pytest.mark.parametrize("source", ["synth", "rand"])
@pytest.mark.parametrize("W,H,half", aux_np.NOVEL_SIZES)
def test_novel_planes_change_the_result(W, H, half, source):
    """Each plane of the content list, replaced by the plane of py -- which a
    named code expresses --, gives another output: the plane's content reaches
    the result.  The object-id plane takes both arms of scale()."""
    recs = aux_np.novel_frames(W, H, half, source)
    for rec in recs:
        assert np.isfinite(rec["weights"]).all() and np.isfinite(rec["result"]).all()
    for k, nm in enumerate(aux_np.NOVEL_NAMES):
        names = list(aux_np.NOVEL_NAMES)
        names[k] = "py"
        other = aux_np.run(aux_np.AuxOracleLoop(W, H, aux_np.NOVEL_NOT_SCALED, aux_np.NOVEL_SCALED, half, names),
                           source, aux_np.NOVEL_FRAMES)
        d = rel_l2(recs[-1]["result"], other[-1]["result"])
        print(f"{W}x{H} half={half} {source}: without {nm}, result moves by rel-L2 {d:.3e}")
        assert recs[-1]["result"].tobytes() != other[-1]["result"].tobytes() and d > 1e-6, (nm, d)
    slot = aux_np.NOVEL_SCALED.index(AUX0 + aux_np.NOVEL_NAMES.index("objid"))
    flat = across = 0
    for rec in recs:
        mm = rec["mins_maxs"].reshape(-1, len(aux_np.NOVEL_SCALED), 2)[:, slot]
        d = mm[:, 1] - mm[:, 0]
        flat += int((d == 0).sum())
        across += int((np.abs(d) > 1).sum())
    assert flat > 0 and across > 0, (flat, across)
