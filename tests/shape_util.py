"""Shared by the shape sweep's tests (ref_configs.SHAPE_REF_CONFIGS;
tests/test_shapes_cpu.py, tests/test_gpu_shapes.py): the sweep's content, the
CPU oracle over it, and the aux substitution of each configuration.  TEST
INFRASTRUCTURE ONLY."""
from __future__ import annotations

import aux_np
import pyoracle
import scenes_np
from ref_configs import SHAPE_REF_CONFIGS, SHAPE_SCENE

NAMES = list(SHAPE_REF_CONFIGS)
NAME_OF = {code: nm for nm, code in aux_np.CODE_OF.items()}


def canonical(not_scaled, scaled) -> bool:
    """What the library's fused_supported() accepts: the lists that run the
    specialised K1 instead of a generic-count kernel."""
    return tuple(not_scaled) == (0, 1, 2, 3) and tuple(scaled) in ((4, 5, 6, 7, 8, 9), tuple(range(4, 13)))


def frame(name: str, f: int) -> dict:
    """Frame f of the configuration's content (scenes_np.frame: shared, read-only)."""
    rc = SHAPE_REF_CONFIGS[name]
    return scenes_np.frame(SHAPE_SCENE, rc.width, rc.height, f, rc.seed)


def run_loop(loop, name: str, frames=None, **kw):
    rc = SHAPE_REF_CONFIGS[name]
    return scenes_np.run_loop(loop, SHAPE_SCENE, rc.width, rc.height, frames or rc.frames, rc.seed, **kw)


_oracle = {}


def oracle_frames(name: str, codes=None, frames=None):
    """The CPU oracle's records over the configuration's frames, computed once
    and never modified.  codes: another list of the same counts (not_scaled +
    scaled) in place of the configuration's; such a run is not kept."""
    rc = SHAPE_REF_CONFIGS[name]
    ns = len(rc.not_scaled)

    def run(codes):
        cfg = pyoracle.make_cfg(rc.width, rc.height, codes[:ns], codes[ns:], rc.half_tmp, **rc.knobs())
        return run_loop(pyoracle.OracleLoop(cfg), name, frames)
    if codes is not None or frames is not None:
        return run(tuple(codes) if codes is not None else rc.not_scaled + rc.scaled)
    if name not in _oracle:
        _oracle[name] = run(rc.not_scaled + rc.scaled)
    return _oracle[name]


def forget(name: str) -> None:
    """Drop the configuration's kept records (a caller that goes through the
    sweep one configuration at a time)."""
    _oracle.pop(name, None)


def aux_case(name: str):
    """The configuration's list with the last position and, where NS >= 2,
    position 1 replaced by caller-supplied planes; the plane index rotates
    with the shape.  -> (not_scaled, scaled, names): names[k] is the
    aux_np.PLANES key of the monomial plane k holds (None: not named)."""
    return aux_case_of(SHAPE_REF_CONFIGS[name])


def aux_case_of(rc):
    """aux_case for any configuration with a generic (non-canonical) list."""
    ns = len(rc.not_scaled)
    codes = rc.not_scaled + rc.scaled
    k = (ns + len(rc.scaled)) % 4
    subs = {len(codes) - 1: k}
    if ns >= 2 and len(codes) > 2:
        subs[1] = (k + 1) % 4
    out, was = aux_np.substitute(codes, subs)
    names = tuple(NAME_OF[was[i]] if i in was else None for i in range(4))
    return out[:ns], out[ns:], names
