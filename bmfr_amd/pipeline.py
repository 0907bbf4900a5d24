"""Host-side mirror of the reference's frame driver over libbmfr's C ABI.

Reference: tasks() in /root/reference/opencl/bmfr.cpp:179-556.

* `BmfrConfig` is the `#define` surface of bmfr.cpp:32-118.
* `StagePipeline` replays tasks()' frame loop (bmfr.cpp:417-485) one stage at
  a time on torch-owned device buffers laid out like the reference's
  cl::Buffers (bmfr.cpp:315-347), including the Double_buffer swap
  (bmfr.cpp:122-135, 482-484).  It exists so every intermediate buffer can be
  compared with the reference kernels and the CPU oracle.
* `Denoiser` is the production path: one `bmfr_process_frame` per frame
  (fused K1 + TAA), temporal state owned by the C context.

Device memory, streams and copies come from torch; the compute is libbmfr's
HIP kernels.  Nothing here falls back to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import torch

from . import _lib
from ._lib import check, floats

NOT_SCALED_DEFAULT = (_lib.FEATURE_ONE, _lib.NORMAL_X, _lib.NORMAL_Y, _lib.NORMAL_Z)
SCALED_DEFAULT = (_lib.POSITION_X, _lib.POSITION_Y, _lib.POSITION_Z,
                  _lib.POSITION_X2, _lib.POSITION_Y2, _lib.POSITION_Z2)
SCALED_THIRD_ORDER = SCALED_DEFAULT + (_lib.POSITION_X3, _lib.POSITION_Y3, _lib.POSITION_Z3)


@dataclasses.dataclass(frozen=True)
class BmfrConfig:
    """bmfr.cpp's compile-time parameters (names follow the #defines)."""
    image_width: int = 1280                  # IMAGE_WIDTH  bmfr.cpp:39
    image_height: int = 720                  # IMAGE_HEIGHT bmfr.cpp:40
    not_scaled: tuple = NOT_SCALED_DEFAULT   # NOT_SCALED_FEATURE_BUFFERS bmfr.cpp:65-69
    scaled: tuple = SCALED_DEFAULT           # SCALED_FEATURE_BUFFERS bmfr.cpp:71-77
    noise_amount: float = 1e-2               # NOISE_AMOUNT bmfr.cpp:58
    blend_alpha: float = 0.2                 # BLEND_ALPHA bmfr.cpp:60
    second_blend_alpha: float = 0.1          # SECOND_BLEND_ALPHA bmfr.cpp:61
    taa_blend_alpha: float = 0.2             # TAA_BLEND_ALPHA bmfr.cpp:62
    position_limit_squared: float = 0.01     # camera_matrices.h, bmfr.cpp:226
    normal_limit_squared: float = 0.1        # camera_matrices.h, bmfr.cpp:227
    use_half_precision_in_tmp_data: int = 1  # bmfr.cpp:88
    # Multi-GPU tile of the frame (include/bmfr.h: tile_*): (x, y, width, height), halo
    tile: tuple | None = None
    tile_halo: int = 0
    # Frame input planes in IEEE half (half3, 6 B/px) instead of f32 (include/bmfr.h: input_half)
    input_half: int = 0
    # Tone map powr: 0 = correctly rounded (== the CPU oracle), 1 = the device
    # library's powr (== the reference kernel on gfx950) (include/bmfr.h: library_powr)
    library_powr: int = 0
    # Householder trailing update as one fused FMA, butterfly reductions, hardware sqrt / rcp on
    # the pivot chain (not bit-exact: measured <= 1.2e-5 rel-L2 of the reference's strict build
    # at 4K, 3.0e-5 at B = 16; the tests hold it to north_star's 1e-4; fused K1, canonical
    # feature lists) (include/bmfr.h: fast_fit)
    fast_fit: int = 0

    @property
    def buffer_count(self) -> int:
        return len(self.not_scaled) + len(self.scaled) + 3

    def to_c(self) -> _lib.Config:
        lib = _lib.load()
        c = _lib.Config()
        lib.bmfr_config_default(C.byref(c), self.image_width, self.image_height)
        feats = tuple(self.not_scaled) + tuple(self.scaled)
        c.features_not_scaled = len(self.not_scaled)
        c.features_scaled = len(self.scaled)
        for i in range(_lib.MAX_FEATURES):
            c.feature_buffers[i] = feats[i] if i < len(feats) else 0
        c.noise_amount = self.noise_amount
        c.blend_alpha = self.blend_alpha
        c.second_blend_alpha = self.second_blend_alpha
        c.taa_blend_alpha = self.taa_blend_alpha
        c.position_limit_squared = self.position_limit_squared
        c.normal_limit_squared = self.normal_limit_squared
        c.use_half_precision_in_tmp_data = self.use_half_precision_in_tmp_data
        if self.tile is not None:
            c.tile_x, c.tile_y, c.tile_width, c.tile_height = self.tile
            c.tile_halo = self.tile_halo
        c.input_half = self.input_half
        c.library_powr = self.library_powr
        c.fast_fit = self.fast_fit
        return c

    def sizes(self) -> _lib.Sizes:
        s = _lib.Sizes()
        check(_lib.load().bmfr_config_sizes(C.byref(self.to_c()), C.byref(s)), "bmfr_config_sizes")
        return s


def _ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


def check_prev_pixel(plane, width: int, height: int, device: int = 0) -> None:
    """Raise unless `plane` can be passed as bmfr_frame_inputs.prev_pixel
    (include/bmfr.h) of a context whose planes cover width x height pixels (the
    image, or a tiled context's region) on GPU `device`: a contiguous float32
    tensor of shape (height, width, 2) or (height * width * 2,) there.  None
    (project with the camera matrix) passes.  Runs before any library call,
    which would read a wrong plane out of bounds."""
    if plane is None:
        return
    if not isinstance(plane, torch.Tensor):
        raise TypeError(f"prev_pixel must be a torch tensor or None, not {type(plane).__name__}")
    if plane.dtype != torch.float32:
        raise TypeError(f"prev_pixel must be float32 (also with input_half), not {plane.dtype}")
    if tuple(plane.shape) not in ((height, width, 2), (height * width * 2,)):
        raise ValueError(f"prev_pixel must have shape ({height}, {width}, 2) or ({height * width * 2},), "
                         f"not {tuple(plane.shape)}")
    if not plane.is_contiguous():
        raise ValueError("prev_pixel must be contiguous")
    if plane.device.type != "cuda" or (plane.device.index or 0) != device:
        raise ValueError(f"prev_pixel must live on cuda:{device}, not {plane.device}")


def aux_named(cfg: "BmfrConfig") -> tuple:
    """The aux plane indices (0..3) the configuration's feature lists name."""
    feats = tuple(cfg.not_scaled) + tuple(cfg.scaled)
    return tuple(k for k in range(_lib.MAX_AUX_FEATURES) if _lib.FEATURE_AUX0 + k in feats)


def check_aux(aux, named, width: int, height: int, device: int = 0) -> tuple:
    """Raise unless `aux` can be passed as bmfr_aux_inputs.aux (include/bmfr.h)
    of a context whose feature lists name the planes `named` (aux_named) and
    whose planes cover width x height pixels on GPU `device`: None, or a
    sequence of up to four entries, each None or a contiguous float32 tensor of
    height * width elements there; every named plane must be present.  Runs
    before any library call, which would read a wrong plane out of bounds.
    -> the four entries (None where absent)."""
    if aux is None:
        aux = ()
    if isinstance(aux, torch.Tensor) or not hasattr(aux, "__len__"):
        raise TypeError("aux must be a sequence of up to four tensors or Nones")
    if len(aux) > _lib.MAX_AUX_FEATURES:
        raise ValueError(f"aux takes at most {_lib.MAX_AUX_FEATURES} planes, not {len(aux)}")
    planes = tuple(aux) + (None,) * (_lib.MAX_AUX_FEATURES - len(aux))
    for k in named:
        if planes[k] is None:
            raise ValueError(f"the feature list names FEATURE_AUX{k} but aux[{k}] is missing")
    for k, t in enumerate(planes):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"aux[{k}] must be a torch tensor or None, not {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"aux[{k}] must be float32, not {t.dtype}")
        if t.numel() != height * width:
            raise ValueError(f"aux[{k}] must have {height * width} elements ({height} x {width}), "
                             f"not {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"aux[{k}] must be contiguous")
        if t.device.type != "cuda" or (t.device.index or 0) != device:
            raise ValueError(f"aux[{k}] must live on cuda:{device}, not {t.device}")
    return planes


def _stream(stream) -> int | None:
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


class _Context:
    def __init__(self, cfg: BmfrConfig, device: int = 0):
        self.cfg = cfg
        self.lib = _lib.load()
        self.device = device
        h = C.c_void_p()
        check(self.lib.bmfr_create(C.byref(cfg.to_c()), device, C.byref(h)), "bmfr_create")
        self.handle = h
        self.sizes = cfg.sizes()

    def close(self) -> None:
        if self.handle:
            self.lib.bmfr_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StagePipeline(_Context):
    """The reference frame loop, stage by stage, on reference-layout buffers."""

    def __init__(self, cfg: BmfrConfig, device: int = 0):
        if aux_named(cfg):
            raise ValueError("StagePipeline cannot run a feature list that names FEATURE_AUX planes: the stage "
                             "API keeps the reference's kernel signatures, which have no aux argument "
                             "(bmfr_accumulate_noisy_data / bmfr_weighted_sum: unsupported); use Denoiser")
        super().__init__(cfg, device)
        dev = torch.device("cuda", device)
        W, H = cfg.image_width, cfg.image_height
        s = self.sizes
        f32 = dict(dtype=torch.float32, device=dev)
        img = lambda: torch.zeros(H * W * 3, **f32)  # noqa: E731
        self.normals = [img(), img()]
        self.positions = [img(), img()]
        self.noisy = [img(), img()]
        self.out = [img(), img()]          # accumulated filtered colour
        self.result = [img(), img()]       # TAA output
        self.spp = [torch.zeros(H * W, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.albedo = img()
        self.filtered = img()
        self.tone_mapped = img()
        self.prev_pixels = torch.zeros(H * W * 2, **f32)
        self.accept = torch.zeros(H * W, dtype=torch.uint8, device=dev)
        tmp_elems = s.tmp_data_bytes // (2 if cfg.use_half_precision_in_tmp_data else 4)
        self.tmp_data = torch.zeros(tmp_elems, dtype=torch.float16 if cfg.use_half_precision_in_tmp_data
                                    else torch.float32, device=dev)
        self.weights = torch.zeros(s.weights_bytes // 4, **f32)
        self.mins_maxs = torch.zeros(s.mins_maxs_bytes // 4, **f32)
        self.swapped = False

    def cur(self, pair):
        return pair[0] if self.swapped else pair[1]   # Double_buffer::current, bmfr.cpp:132

    def prev(self, pair):
        return pair[1] if self.swapped else pair[0]   # Double_buffer::previous, bmfr.cpp:133

    def upload(self, noisy, normals, positions, albedo) -> None:
        """enqueueWriteBuffer of bmfr.cpp:420-427 (device-to-device here)."""
        self.cur(self.noisy).copy_(noisy.reshape(-1))
        self.cur(self.normals).copy_(normals.reshape(-1))
        self.cur(self.positions).copy_(positions.reshape(-1))
        self.albedo.copy_(albedo.reshape(-1))

    def run_stages(self, prev_vp, jitter, frame: int, stream=None, record=None) -> None:
        lib, h, st = self.lib, self.handle, _stream(stream)
        vp, jt = floats(prev_vp, 16), floats(jitter, 2)
        check(lib.bmfr_accumulate_noisy_data(
            h, st, _ptr(self.prev_pixels), _ptr(self.accept), _ptr(self.cur(self.normals)),
            _ptr(self.prev(self.normals)), _ptr(self.cur(self.positions)), _ptr(self.prev(self.positions)),
            _ptr(self.cur(self.noisy)), _ptr(self.prev(self.noisy)), _ptr(self.prev(self.spp)),
            _ptr(self.cur(self.spp)), _ptr(self.tmp_data), vp, jt, frame), "accumulate_noisy_data")
        if record is not None:
            record["tmp_noisy"] = self.tmp_data.clone()
        check(lib.bmfr_fitter(h, st, _ptr(self.weights), _ptr(self.mins_maxs), _ptr(self.tmp_data), frame),
              "fitter")
        check(lib.bmfr_weighted_sum(h, st, _ptr(self.weights), _ptr(self.mins_maxs), _ptr(self.filtered),
                                    _ptr(self.cur(self.normals)), _ptr(self.cur(self.positions)),
                                    _ptr(self.cur(self.noisy)), frame), "weighted_sum")
        check(lib.bmfr_accumulate_filtered_data(
            h, st, _ptr(self.filtered), _ptr(self.prev_pixels), _ptr(self.accept), _ptr(self.albedo),
            _ptr(self.tone_mapped), _ptr(self.cur(self.spp)), _ptr(self.prev(self.out)),
            _ptr(self.cur(self.out)), frame), "accumulate_filtered_data")
        check(lib.bmfr_taa(h, st, _ptr(self.prev_pixels), _ptr(self.tone_mapped),
                           _ptr(self.cur(self.result)), _ptr(self.prev(self.result)), frame), "taa")
        if record is not None:
            record.update(
                tmp_fit=self.tmp_data.clone(), weights=self.weights.clone(),
                mins_maxs=self.mins_maxs.clone(), filtered=self.filtered.clone(),
                acc=self.cur(self.out).clone(), tone=self.tone_mapped.clone(),
                result=self.cur(self.result).clone(), spp=self.cur(self.spp).clone(),
                accept=self.accept.clone(), prev_pixel=self.prev_pixels.clone(),
                noisy=self.cur(self.noisy).clone())

    def swap(self) -> None:
        self.swapped = not self.swapped             # bmfr.cpp:482-484


class Denoiser(_Context):
    """Production path: one fused `bmfr_process_frame` per frame."""

    def __init__(self, cfg: BmfrConfig, device: int = 0):
        super().__init__(cfg, device)
        self.prev_inputs = None

    def _check_prev_pixel(self, plane) -> None:
        check_prev_pixel(plane, self.sizes.region_width, self.sizes.region_height, self.device)

    def _check_aux(self, aux):
        """-> the frame's bmfr_aux_inputs (checked: check_aux)."""
        planes = check_aux(aux, aux_named(self.cfg), self.sizes.region_width, self.sizes.region_height, self.device)
        return _lib.AuxInputs((C.c_void_p * _lib.MAX_AUX_FEATURES)(*[_ptr(t) for t in planes]))

    def _call(self, fn: str, noisy, normals, positions, albedo, prev_vp, jitter, frame, prev_normals,
              prev_positions, stream, done: bool, prev_pixel=None, aux=None) -> None:
        self._check_prev_pixel(prev_pixel)
        aux_c = self._check_aux(aux)
        if frame > 0 and prev_normals is None:
            if self.prev_inputs is None:
                raise ValueError("frame > 0 needs the previous frame's normals/positions")
            prev_normals, prev_positions = self.prev_inputs
        fi = _lib.FrameInputs(_ptr(noisy), _ptr(normals), _ptr(positions), _ptr(albedo),
                              _ptr(prev_normals), _ptr(prev_positions), _ptr(prev_pixel))
        if aux_named(self.cfg):  # the call with the planes; every other configuration calls what it always did
            check(getattr(self.lib, fn + "_aux")(self.handle, _stream(stream), C.byref(fi), C.byref(aux_c),
                                                 floats(prev_vp, 16), floats(jitter, 2), frame), fn + "_aux")
        else:
            check(getattr(self.lib, fn)(self.handle, _stream(stream), C.byref(fi), floats(prev_vp, 16),
                                        floats(jitter, 2), frame), fn)
        if done:
            self.prev_inputs = (normals, positions)

    def process_frame(self, noisy, normals, positions, albedo, prev_vp, jitter, frame: int,
                      prev_normals=None, prev_positions=None, stream=None, prev_pixel=None, aux=None) -> None:
        """Run one frame.  prev_normals / prev_positions default to the ones
        passed on the previous call (the reference's Double_buffer halves).
        prev_pixel: optional float32 (H, W, 2) plane of previous-frame pixel
        positions that replaces the projection through prev_vp from frame 1 on
        (include/bmfr.h bmfr_frame_inputs.prev_pixel; the region for a tile).
        aux: a sequence of up to four float32 (H, W) planes or Nones, the
        values of the features FEATURE_AUX0..3 at this frame's pixels
        (include/bmfr.h bmfr_aux_inputs); every plane the configuration
        names must be there."""
        self._call("bmfr_process_frame", noisy, normals, positions, albedo, prev_vp, jitter, frame,
                   prev_normals, prev_positions, stream, True, prev_pixel, aux)

    def process_sequence(self, frames, cameras, first_frame: int, outputs=None, stream=None) -> None:
        """Frames first_frame .. first_frame+len(frames)-1 in one pipelined call
        (include/bmfr.h bmfr_process_sequence).  frames: dicts with noisy,
        normals, positions, albedo tensors and optionally prev_pixel (a plane
        as in process_frame, or None), aux (as in process_frame) and prev_normals / prev_positions
        (default: the frame before's normals / positions); cameras: (prev_vp,
        jitter) per frame; outputs: optional tensors receiving each frame's
        output."""
        n = len(frames)
        arr = (_lib.FrameInputs * n)()
        aux_arr = (_lib.AuxInputs * n)()
        prev = self.prev_inputs
        for i, fr in enumerate(frames):
            pn, pp = prev if prev is not None else (None, None)
            if fr.get("prev_normals") is not None:
                pn, pp = fr["prev_normals"], fr["prev_positions"]
            self._check_prev_pixel(fr.get("prev_pixel"))
            arr[i] = _lib.FrameInputs(_ptr(fr["noisy"]), _ptr(fr["normals"]), _ptr(fr["positions"]),
                                      _ptr(fr["albedo"]), _ptr(pn), _ptr(pp), _ptr(fr.get("prev_pixel")))
            aux_arr[i] = self._check_aux(fr.get("aux"))
            prev = (fr["normals"], fr["positions"])
        vps = floats([v for vp, _ in cameras for v in vp], 16 * n)
        offs = floats([v for _, jit in cameras for v in jit], 2 * n)
        outs = None
        if outputs is not None:
            outs = (C.c_void_p * n)(*[_ptr(o) for o in outputs])
        if aux_named(self.cfg):
            check(self.lib.bmfr_process_sequence_aux(self.handle, _stream(stream), n, arr, aux_arr, vps, offs,
                                                     first_frame, outs), "bmfr_process_sequence_aux")
        else:
            check(self.lib.bmfr_process_sequence(self.handle, _stream(stream), n, arr, vps, offs, first_frame, outs),
                  "bmfr_process_sequence")
        self.prev_inputs = prev

    def process_frame_interior(self, noisy, normals, positions, albedo, prev_vp, jitter, frame: int,
                               prev_normals=None, prev_positions=None, stream=None, prev_pixel=None,
                               aux=None) -> None:
        """First half of a frame (include/bmfr.h): the K1 blocks that need no
        halo; may run while the halo exchange of the previous state is in flight."""
        self._call("bmfr_process_frame_interior", noisy, normals, positions, albedo, prev_vp, jitter, frame,
                   prev_normals, prev_positions, stream, False, prev_pixel, aux)

    def process_frame_border(self, noisy, normals, positions, albedo, prev_vp, jitter, frame: int,
                             prev_normals=None, prev_positions=None, stream=None, prev_pixel=None,
                             aux=None) -> None:
        """Second half: the remaining K1 blocks and K2, once the halo is refreshed."""
        self._call("bmfr_process_frame_border", noisy, normals, positions, albedo, prev_vp, jitter, frame,
                   prev_normals, prev_positions, stream, True, prev_pixel, aux)

    # ---- G-buffer front end (include/bmfr.h bmfr_prepare_frame) ----
    # g key -> (bmfr_gbuffer format field, {tensor dtype: (bmfr_format, elements per pixel)})
    _GBUFFER_PLANES = {
        "radiance": ("radiance_format", {torch.float32: (_lib.FORMAT_F32X3, 3), torch.float16: (_lib.FORMAT_F16X4, 4)}),
        "albedo": ("albedo_format", {torch.float32: (_lib.FORMAT_F32X3, 3), torch.float16: (_lib.FORMAT_F16X4, 4),
                                     torch.uint8: (_lib.FORMAT_UNORM8X4, 4)}),
        "normals": ("normal_format", {torch.float32: (_lib.FORMAT_F32X3, 3), torch.float16: (_lib.FORMAT_F16X4, 4),
                                      torch.int16: (_lib.FORMAT_OCT_SNORM16X2, 2)}),
        "motion": ("motion_format", {torch.float32: (_lib.FORMAT_F32X2, 2), torch.float16: (_lib.FORMAT_F16X2, 2)}),
        "positions": (None, {torch.float32: (None, 3)}),
        "depth": (None, {torch.float32: (None, 1)}),
        "prev_object_id": (None, {torch.int16: (None, 1), getattr(torch, "uint16", torch.int16): (None, 1)}),
    }
    _PREPARED = ("noisy", "normals", "positions", "albedo", "prev_pixel", "prev_positions_moved",
                 "prev_normals_moved")

    def _check_plane(self, name: str, t, dtypes, pixels: int | None = None):
        """A plane handed to the library: a contiguous tensor on this GPU of
        one of `dtypes` (dtype -> (format, elements per pixel)) covering the
        region (or `pixels` pixels).  Runs before the call, which would read a
        wrong plane out of bounds.  -> the dtype's format."""
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, not {type(t).__name__}")
        if t.dtype not in dtypes:
            raise TypeError(f"{name} must be one of {[str(d) for d in dtypes]}, not {t.dtype}")
        fmt, per = dtypes[t.dtype]
        n = (self.sizes.region_width * self.sizes.region_height if pixels is None else pixels) * per
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous with {n} elements, not {tuple(t.shape)}")
        if t.device.type != "cuda" or (t.device.index or 0) != self.device:
            raise ValueError(f"{name} must live on cuda:{self.device}, not {t.device}")
        return fmt

    def prepare(self, g: dict, jitter, out: dict | None = None, stream=None) -> dict:
        """bmfr_prepare_frame: a renderer's G-buffer -> the planes process_frame
        takes, in one kernel launch (arguments: prepare_args).  -> out."""
        gb, pr, out = self.prepare_args(g, out)
        check(self.lib.bmfr_prepare_frame(self.handle, _stream(stream), C.byref(gb), C.byref(pr), floats(jitter, 2)),
              "bmfr_prepare_frame")
        return out

    def prepare_args(self, g: dict, out: dict | None = None):
        """The checked arguments of bmfr_prepare_frame -> (bmfr_gbuffer,
        bmfr_prepared, out); a caller that repeats a call keeps them.  g: tensors over the region by name --
        radiance, albedo, normals, positions or depth (with inv_view_proj, 16
        floats column-major), motion, prev_positions, prev_normals,
        prev_object_id (int16 / uint16 bits), object_transforms (float32,
        12 per object) -- and the scalars albedo_floor, motion_scale,
        motion_at_pixel_centre; a plane's format follows from its dtype
        (float32 / float16 = RGBA16F or RG16F / uint8 = UNORM8X4 / int16 =
        octahedral).  out: the outputs to compute by name (noisy, normals,
        positions, albedo, prev_pixel, prev_positions_moved,
        prev_normals_moved); None: every output whose inputs are in g,
        allocated in the context's input format."""
        gb = _lib.GBuffer()
        self.lib.bmfr_gbuffer_default(C.byref(gb))
        for name, (fmt_field, dtypes) in self._GBUFFER_PLANES.items():
            t = g.get(name)
            if t is None:
                continue
            fmt = self._check_plane(name, t, dtypes)
            setattr(gb, name, t.data_ptr())
            if fmt_field:
                setattr(gb, fmt_field, fmt)
        plane_dtype = torch.float16 if self.cfg.input_half else torch.float32
        for name in ("prev_positions", "prev_normals"):
            if g.get(name) is not None:
                self._check_plane(name, g[name], {plane_dtype: (None, 3)})
                setattr(gb, name, g[name].data_ptr())
        tr = g.get("object_transforms")
        if tr is not None:
            if not isinstance(tr, torch.Tensor) or tr.dtype != torch.float32 or tr.numel() % 12 or \
                    not tr.is_contiguous() or tr.device.type != "cuda" or (tr.device.index or 0) != self.device:
                raise ValueError("object_transforms must be a contiguous float32 tensor of 12 floats per object "
                                 f"on cuda:{self.device}")
            gb.object_transforms, gb.n_objects = tr.data_ptr(), tr.numel() // 12
        if g.get("inv_view_proj") is not None:
            gb.inv_view_proj[:] = [float(v) for v in g["inv_view_proj"]]
        if "albedo_floor" in g:
            gb.albedo_floor = g["albedo_floor"]
        if "motion_scale" in g:
            gb.motion_scale[:] = [float(v) for v in g["motion_scale"]]
        gb.motion_at_pixel_centre = int(g.get("motion_at_pixel_centre", 0))
        if out is None:
            has = lambda *names: all(g.get(n) is not None for n in names)  # noqa: E731
            want = {"noisy": has("radiance", "albedo"), "albedo": has("albedo"), "normals": has("normals"),
                    "positions": has("positions") or has("depth"), "prev_pixel": has("motion"),
                    "prev_positions_moved": has("prev_positions"), "prev_normals_moved": has("prev_normals")}
            n = self.sizes.region_width * self.sizes.region_height
            dev = torch.device("cuda", self.device)
            out = {k: torch.empty(n * 2, dtype=torch.float32, device=dev) if k == "prev_pixel" else
                   torch.empty(n * 3, dtype=plane_dtype, device=dev) for k, w in want.items() if w}
        pr = _lib.Prepared()
        for name, t in out.items():
            if name not in self._PREPARED:
                raise KeyError(f"unknown prepared plane {name!r}")
            self._check_plane(name, t, {torch.float32: (None, 2)} if name == "prev_pixel" else {plane_dtype: (None, 3)})
            setattr(pr, name, t.data_ptr())
        return gb, pr, out

    # ---- Firefly pre-filter (include/bmfr.h bmfr_suppress_fireflies) ----
    def firefly_args(self, noisy, out=None, threshold=2.0, radius=1, floor=0.0, replace_nonfinite=True, stats=None):
        """The checked arguments of bmfr_suppress_fireflies -> (out,
        bmfr_firefly_params); a caller that repeats a call keeps them.  Runs
        before the call, which would read or write a wrong plane out of bounds."""
        dtypes = {torch.float16 if self.cfg.input_half else torch.float32: (None, 3)}
        self._check_plane("noisy", noisy, dtypes)
        if out is None:
            out = torch.empty_like(noisy)
        self._check_plane("out", out, dtypes)
        if stats is not None:
            if not isinstance(stats, torch.Tensor) or stats.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) \
                    or stats.numel() != 2 or not stats.is_contiguous() or stats.device.type != "cuda" \
                    or (stats.device.index or 0) != self.device:
                raise ValueError(f"stats must be a contiguous tensor of two 32-bit integers on cuda:{self.device}")
        p = _lib.FireflyParams()
        self.lib.bmfr_firefly_default(C.byref(p))
        p.threshold, p.radius, p.floor = float(threshold), int(radius), float(floor)
        p.replace_nonfinite = int(bool(replace_nonfinite))
        return out, p

    def suppress_fireflies(self, noisy, out=None, threshold=2.0, radius=1, floor=0.0, replace_nonfinite=True,
                           stats=None, stream=None):
        """bmfr_suppress_fireflies: the noisy plane (the region; float3, or
        half3 with input_half) with every pixel held to `threshold` times its
        brightest neighbour within `radius` (1 or 2), never below the luminance
        `floor`, and pixels with a NaN / inf channel zeroed
        (replace_nonfinite), into `out` (default: a new plane; never `noisy`
        itself) in one kernel launch.  stats: an int32 tensor of two counters,
        {clamped, replaced}, which the call adds to.  -> out."""
        out, p = self.firefly_args(noisy, out, threshold, radius, floor, replace_nonfinite, stats)
        check(self.lib.bmfr_suppress_fireflies(self.handle, _stream(stream), _ptr(noisy), _ptr(out), C.byref(p),
                                               _ptr(stats)), "bmfr_suppress_fireflies")
        return out

    def process_gbuffer(self, g: dict, prev_vp, jitter, frame: int, stream=None, firefly=None) -> None:
        """prepare(g), then process_frame on the prepared planes.  The
        denoiser owns two sets of prepared planes and alternates them: K1 of
        frame f + 1 reads frame f's normals and positions, which must stay
        unmodified until then.  From frame 1 on: with object_transforms or
        prev_object_id in g, last frame's planes moved by them are the
        previous planes, else last frame's planes as they are; with motion in
        g, the prepared prev_pixel replaces the projection through prev_vp.
        firefly: a dict of suppress_fireflies' parameters (threshold, radius,
        floor, replace_nonfinite, stats; {} = the defaults): the prepared
        noisy plane goes through the filter, into a third plane the denoiser
        owns, before process_frame reads it.  None: no filter, the launches
        of a call without it."""
        n = self.sizes.region_width * self.sizes.region_height
        if getattr(self, "_prepared_sets", None) is None:
            dev = torch.device("cuda", self.device)
            dt = torch.float16 if self.cfg.input_half else torch.float32
            self._prepared_sets = [{k: torch.empty(n * (2 if k == "prev_pixel" else 3),
                                                   dtype=torch.float32 if k == "prev_pixel" else dt, device=dev)
                                    for k in self._PREPARED} for _ in range(2)]
        cur, last = self._prepared_sets[frame % 2], self._prepared_sets[1 - frame % 2]
        g = dict(g)
        want = ["noisy", "normals", "positions", "albedo"]
        moving = g.get("object_transforms") is not None or g.get("prev_object_id") is not None
        prev_normals, prev_positions, prev_pixel = last["normals"], last["positions"], None
        if frame > 0:
            if moving:
                g["prev_positions"], g["prev_normals"] = last["positions"], last["normals"]
                want += ["prev_positions_moved", "prev_normals_moved"]
                prev_positions, prev_normals = cur["prev_positions_moved"], cur["prev_normals_moved"]
            if g.get("motion") is not None:
                want.append("prev_pixel")
                prev_pixel = cur["prev_pixel"]
        self.prepare(g, jitter, out={k: cur[k] for k in want}, stream=stream)
        noisy = cur["noisy"]
        if firefly is not None:
            if getattr(self, "_filtered_noisy", None) is None:
                self._filtered_noisy = torch.empty_like(noisy)
            noisy = self.suppress_fireflies(noisy, out=self._filtered_noisy, stream=stream, **firefly)
        self.process_frame(noisy, cur["normals"], cur["positions"], cur["albedo"], prev_vp, jitter, frame,
                           prev_normals=prev_normals if frame > 0 else None,
                           prev_positions=prev_positions if frame > 0 else None, stream=stream,
                           prev_pixel=prev_pixel, aux=g.get("aux"))

    def halo_status(self) -> int:
        """Tiled contexts: waits for the last frame; the largest distance (px)
        by which a frame since frame 0 reprojected past its valid state (0 =
        none).  Raises BmfrError (status HALO_EXCEEDED) when it is > 0."""
        v = C.c_uint()
        check(self.lib.bmfr_halo_status(self.handle, C.byref(v)), "bmfr_halo_status")
        return v.value

    def frame_status(self) -> int:
        """Waits for the last enqueued frame; the context's sticky report
        (include/bmfr.h bmfr_frame_status) as a status code, 0 = ok."""
        return self.lib.bmfr_frame_status(self.handle)

    def debug_sync(self, max_polls: int = -1, k1_delay: int = 0) -> None:
        """include/bmfr_debug.h bmfr_debug_sync: the kernels' wait bounds and
        a K1 completion delay, for the frames enqueued from now on."""
        check(self.lib.bmfr_debug_sync(self.handle, max_polls, k1_delay), "bmfr_debug_sync")

    def debug_frame_launches(self, launches: int = 0) -> None:
        """include/bmfr_debug.h bmfr_debug_frame_launches: 0 by frame size (default),
        1 one launch, 2 K1 then K2, for the untiled frames enqueued from now on."""
        check(self.lib.bmfr_debug_frame_launches(self.handle, launches), "bmfr_debug_frame_launches")

    def set_profiling(self, enable: bool, capacity: int = 4096, stride: int = 1) -> None:
        """stride: record only frames whose number is a multiple of it."""
        check(self.lib.bmfr_set_profiling_stride(self.handle, stride), "bmfr_set_profiling_stride")
        check(self.lib.bmfr_set_profiling(self.handle, int(enable), capacity), "bmfr_set_profiling")

    def profile(self):
        """Per-frame device timings [(frame, k1_ms, taa_ms, total_ms)] since profiling was enabled."""
        n = C.c_int()
        check(self.lib.bmfr_get_profile(self.handle, None, 0, C.byref(n)), "bmfr_get_profile")
        buf = (_lib.FrameProfile * 65536)()
        check(self.lib.bmfr_get_profile(self.handle, buf, 65536, C.byref(n)), "bmfr_get_profile")
        return [(p.frame_number, p.fused_block_ms, p.taa_ms, p.total_ms) for p in buf[:n.value]]

    def state(self, previous: bool = False) -> _lib.StateView:
        v = _lib.StateView()
        check(self.lib.bmfr_state(self.handle, int(previous), C.byref(v)), "bmfr_state")
        return v

    def output_ptr(self) -> int:
        p = self.lib.bmfr_output(self.handle)
        if not p:
            raise RuntimeError("no frame processed yet")
        return p

    def copy_output(self, dst: torch.Tensor, stream=None) -> torch.Tensor:
        """Copy the last frame's TAA output (float3 over the buffer region:
        W*H, or a tile's region) into `dst`."""
        hip_memcpy_d2d(dst.data_ptr(), self.output_ptr(), self.sizes.region_bytes, stream)
        return dst

    # ---- Output back end (include/bmfr.h bmfr_resolve_output) ----
    # (dst dtype, channels; None = a 2-D tensor) -> bmfr_format
    _SURFACE_FORMATS = {(torch.uint8, 4): _lib.FORMAT_UNORM8X4, (torch.uint8, 3): _lib.FORMAT_UNORM8X3,
                        (torch.float16, 4): _lib.FORMAT_F16X4, (torch.float32, 3): _lib.FORMAT_F32X3,
                        (torch.int32, None): _lib.FORMAT_UNORM10X3A2}
    _RESOLVE_SOURCES = {"output": _lib.RESOLVE_OUTPUT, "hdr": _lib.RESOLVE_HDR}

    def resolve_args(self, dst, source="output", albedo=None, origin=(0, 0), flip_y=False, bgr=False, alpha=1.0):
        """The checked arguments of bmfr_resolve_output -> (source code, albedo
        pointer, bmfr_surface); a caller that repeats a call keeps them.  Runs
        before the call, which would write a wrong surface out of bounds."""
        s = self._surface(dst, origin, flip_y, bgr, alpha)
        if source not in self._RESOLVE_SOURCES:
            raise ValueError(f"source must be one of {sorted(self._RESOLVE_SOURCES)}, not {source!r}")
        if source == "hdr":
            if albedo is None:
                raise ValueError("source 'hdr' needs the frame's albedo plane")
            self._check_plane("albedo", albedo, {torch.float16 if self.cfg.input_half else torch.float32: (None, 3)})
        self._check_surface_device(dst)
        return self._RESOLVE_SOURCES[source], (_ptr(albedo) if source == "hdr" else None), s

    def _check_surface_device(self, dst) -> None:
        if dst.device.type != "cuda" or (dst.device.index or 0) != self.device:
            raise ValueError(f"dst must live on cuda:{self.device}, not {dst.device}")

    def _surface(self, dst, origin, flip_y, bgr, alpha) -> _lib.Surface:
        """The bmfr_surface of a destination tensor (resolve's docstring); its
        device is checked apart (_check_surface_device)."""
        if not isinstance(dst, torch.Tensor):
            raise TypeError(f"dst must be a torch tensor, not {type(dst).__name__}")
        channels = dst.shape[2] if dst.dim() == 3 else None
        fmt = self._SURFACE_FORMATS.get((dst.dtype, channels)) if dst.dim() in (2, 3) else None
        if fmt is None:
            raise TypeError("dst must be (rows, cols, 4) or (rows, cols, 3) uint8, (rows, cols, 4) float16, "
                            f"(rows, cols, 3) float32 or (rows, cols) int32, not {tuple(dst.shape)} {dst.dtype}")
        inner = (channels, 1) if channels else (1,)
        if dst.numel() == 0 or tuple(dst.stride()[1:]) != inner or dst.stride(0) < dst.shape[1] * (channels or 1):
            raise ValueError(f"dst must have packed pixels and rows that do not overlap (strides {dst.stride()}); "
                             "only its row stride is free")
        s = _lib.Surface()
        self.lib.bmfr_surface_default(C.byref(s))
        s.data, s.format, s.pitch = dst.data_ptr(), fmt, dst.stride(0) * dst.element_size()
        s.width, s.height = dst.shape[1], dst.shape[0]
        s.origin_x, s.origin_y = int(origin[0]), int(origin[1])
        s.flip_y, s.bgr, s.alpha = int(bool(flip_y)), int(bool(bgr)), float(alpha)
        return s

    def resolve(self, dst, source="output", albedo=None, origin=(0, 0), flip_y=False, bgr=False, alpha=1.0,
                stream=None):
        """bmfr_resolve_output: the last frame's tile (never its halo) into the
        surface `dst` in one kernel launch.  dst: a CUDA tensor (rows, cols, C)
        -- uint8 with C = 4 (RGBA8) or 3 (RGB8), float16 with C = 4 (RGBA16F),
        float32 with C = 3 -- or (rows, cols) int32 (R10G10B10A2); its row
        stride is the pitch, so a row- or column-sliced view of a larger tensor
        works.  source: "output" (the TAA result, display-referred) or "hdr"
        (albedo * filtered_accumulated, linear; albedo = the frame's albedo
        plane as given to process_frame).  origin: the surface pixel of frame
        pixel (0, 0), negative for a tile-sized surface.  -> dst."""
        src, alb, s = self.resolve_args(dst, source, albedo, origin, flip_y, bgr, alpha)
        check(self.lib.bmfr_resolve_output(self.handle, _stream(stream), src, alb, C.byref(s)), "bmfr_resolve_output")
        return dst

    # ---- Guided upsampling (include/bmfr.h bmfr_upsample_output) ----
    _UPSAMPLE_SOURCES = {"hdr": _lib.UPSAMPLE_HDR, "tonemapped": _lib.UPSAMPLE_TONEMAPPED}
    # guide -> (format field, dtype -> (format, elements per pixel))
    _GUIDE_PLANES = {
        "albedo": ("albedo_format", {torch.float32: (_lib.FORMAT_F32X3, 3), torch.float16: (_lib.FORMAT_F16X4, 4),
                                     torch.uint8: (_lib.FORMAT_UNORM8X4, 4)}),
        "normals": ("normal_format", {torch.float32: (_lib.FORMAT_F32X3, 3), torch.float16: (_lib.FORMAT_F16X4, 4),
                                      torch.int16: (_lib.FORMAT_OCT_SNORM16X2, 2)}),
        "positions": (None, {torch.float32: (None, 3)}),
        "depth": (None, {torch.float32: (None, 1)}),
    }

    def upsample_args(self, dst, guides: dict, normals=None, positions=None, source="hdr", origin=(0, 0),
                      flip_y=False, bgr=False, alpha=1.0, stats=None):
        """The checked arguments of bmfr_upsample_output -> (source code,
        bmfr_upsample_guides, bmfr_surface); a caller that repeats a call keeps
        them.  Runs before the call, which would read a wrong plane or write a
        wrong surface out of bounds."""
        s = self._surface(dst, origin, flip_y, bgr, alpha)
        if source not in self._UPSAMPLE_SOURCES:
            raise ValueError(f"source must be one of {sorted(self._UPSAMPLE_SOURCES)}, not {source!r}")
        unknown = set(guides) - {f[0] for f in _lib.UpsampleGuides._fields_ if not f[0].endswith("_format")}
        if unknown:
            raise KeyError(f"unknown guide {sorted(unknown)!r}")
        g = _lib.UpsampleGuides()
        self.lib.bmfr_upsample_guides_default(C.byref(g), C.byref(self.cfg.to_c()))
        g.width, g.height = int(guides.get("width", 0)), int(guides.get("height", 0))
        if g.width <= 0 or g.height <= 0:
            raise ValueError("guides need the display size: width and height")
        if guides.get("albedo") is None:
            raise ValueError("guides need the display-resolution albedo plane")
        for name, (fmt_field, dtypes) in self._GUIDE_PLANES.items():
            t = guides.get(name)
            if t is None:
                continue
            fmt = self._check_plane(f"guides[{name!r}]", t, dtypes, pixels=g.width * g.height)
            setattr(g, name, t.data_ptr())
            if fmt_field:
                setattr(g, fmt_field, fmt)
        if guides.get("inv_view_proj") is not None:
            g.inv_view_proj[:] = [float(v) for v in guides["inv_view_proj"]]
        if guides.get("pixel_offset") is not None:
            g.pixel_offset[:] = [float(v) for v in guides["pixel_offset"]]
        for name in ("plane_limit_squared", "normal_limit_squared"):
            if name in guides:
                setattr(g, name, float(guides[name]))
        if guides.get("normals") is not None:   # guided: the frame's own planes
            frame = {torch.float16 if self.cfg.input_half else torch.float32: (None, 3)}
            for name, t in (("normals", normals), ("positions", positions)):
                if t is None:
                    raise ValueError(f"guided upsampling needs the frame's {name} plane")
                self._check_plane(name, t, frame)
        if stats is not None:
            if not isinstance(stats, torch.Tensor) or stats.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) \
                    or stats.numel() != 1 or not stats.is_contiguous() or stats.device.type != "cuda" \
                    or (stats.device.index or 0) != self.device:
                raise ValueError(f"stats must be a contiguous tensor of one 32-bit integer on cuda:{self.device}")
        self._check_surface_device(dst)
        return self._UPSAMPLE_SOURCES[source], g, s

    def upsample(self, dst, guides: dict, normals=None, positions=None, source="hdr", origin=(0, 0), flip_y=False,
                 bgr=False, alpha=1.0, stats=None, stream=None):
        """bmfr_upsample_output: the last frame's filtered_accumulated stretched
        to the display resolution of `guides`, taps on another surface than the
        display pixel left out, times the display-resolution albedo, into the
        surface `dst` (as resolve takes it) in one kernel launch.  guides: the
        renderer's display-resolution G-buffer by the names of
        bmfr_upsample_guides -- width, height, albedo (float32 / float16 =
        RGBA16F / uint8 = UNORM8X4), and for guided mode normals (float32 /
        float16 / int16 = octahedral) with positions or depth (with
        inv_view_proj, 16 floats column-major, and pixel_offset);
        plane_limit_squared / normal_limit_squared default to the
        configuration's limits.  normals, positions: the frame's planes as given
        to process_frame (guided mode).  source: "hdr" (linear) or "tonemapped"
        (display-referred).  stats: an int32 tensor of one counter, the pixels
        none of whose taps passed, which the call adds to.  Untiled contexts
        only.  -> dst."""
        src, g, s = self.upsample_args(dst, guides, normals, positions, source, origin, flip_y, bgr, alpha, stats)
        check(self.lib.bmfr_upsample_output(self.handle, _stream(stream), src, _ptr(normals), _ptr(positions),
                                            C.byref(g), C.byref(s), _ptr(stats)), "bmfr_upsample_output")
        return dst

    # ---- Display-resolution TAA (include/bmfr.h bmfr_display_taa) ----
    # (plane dtype, channels) -> bmfr_format
    _TAA_PLANES = {(torch.float32, 3): _lib.FORMAT_F32X3, (torch.float16, 4): _lib.FORMAT_F16X4}
    _MOTION_FORMATS = {torch.float32: _lib.FORMAT_F32X2, torch.float16: _lib.FORMAT_F16X2}

    def _taa_plane(self, name: str, t, size=None) -> _lib.Plane:
        """The bmfr_plane of a (Hd, Wd, 3) float32 or (Hd, Wd, 4) float16 tensor on
        this GPU, packed pixels, the row stride free."""
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, not {type(t).__name__}")
        fmt = self._TAA_PLANES.get((t.dtype, t.shape[2])) if t.dim() == 3 else None
        if fmt is None:
            raise TypeError(f"{name} must be (rows, cols, 3) float32 or (rows, cols, 4) float16, not "
                            f"{tuple(t.shape)} {t.dtype}")
        ch = t.shape[2]
        if t.numel() == 0 or tuple(t.stride()[1:]) != (ch, 1) or t.stride(0) < t.shape[1] * ch:
            raise ValueError(f"{name} must have packed pixels and rows that do not overlap (strides {t.stride()}); "
                             "only its row stride is free")
        if size is not None and tuple(t.shape[:2]) != size:
            raise ValueError(f"{name} must be {size[0]} x {size[1]} pixels like current, not {tuple(t.shape[:2])}")
        if t.device.type != "cuda" or (t.device.index or 0) != self.device:
            raise ValueError(f"{name} must live on cuda:{self.device}, not {t.device}")
        return _lib.Plane(t.data_ptr(), fmt, t.stride(0) * t.element_size())

    def display_taa_args(self, current, result, history=None, prev_pixel=None, motion=None, motion_scale=(1, 1),
                         motion_at_pixel_centre=False, pixel_offset=(0.5, 0.5), blend_alpha=None, reset=False,
                         dst=None, origin=(0, 0), flip_y=False, bgr=False, alpha=1.0):
        """The checked arguments of bmfr_display_taa -> (bmfr_display_taa_args,
        bmfr_surface or None); a caller that repeats a call keeps them.  Runs
        before the call, which would read a wrong plane or write a wrong surface
        out of bounds."""
        a = _lib.DisplayTaaArgs()
        self.lib.bmfr_display_taa_default(C.byref(a), C.byref(self.cfg.to_c()))
        a.current = self._taa_plane("current", current)
        size = tuple(current.shape[:2])
        a.height, a.width = size
        a.result = self._taa_plane("result", result, size)
        if history is not None:
            a.history = self._taa_plane("history", history, size)
        pixels = a.width * a.height
        if prev_pixel is not None:
            self._check_plane("prev_pixel", prev_pixel, {torch.float32: (None, 2)}, pixels=pixels)
            a.prev_pixel = prev_pixel.data_ptr()
        if motion is not None:
            a.motion_format = self._check_plane("motion", motion, {d: (f, 2) for d, f in self._MOTION_FORMATS.items()},
                                                pixels=pixels)
            a.motion = motion.data_ptr()
        a.motion_scale[:] = [float(v) for v in motion_scale]
        a.motion_at_pixel_centre = int(bool(motion_at_pixel_centre))
        a.pixel_offset[:] = [float(v) for v in pixel_offset]
        if blend_alpha is not None:
            a.blend_alpha = float(blend_alpha)
        a.reset = int(bool(reset))
        s = None
        if dst is not None:
            s = self._surface(dst, origin, flip_y, bgr, alpha)
            self._check_surface_device(dst)
        return a, s

    def display_taa(self, current, result, history=None, prev_pixel=None, motion=None, motion_scale=(1, 1),
                    motion_at_pixel_centre=False, pixel_offset=(0.5, 0.5), blend_alpha=None, reset=False, dst=None,
                    origin=(0, 0), flip_y=False, bgr=False, alpha=1.0, stream=None):
        """bmfr_display_taa: the reference's TAA at display resolution, on
        planes the caller owns, in one kernel launch.  current: this frame's
        display-resolution colour, e.g. the tensor upsample(source=
        "tonemapped") wrote; history: the previous call's result (None: no
        history, as reset); result: written, the next call's history.  Each is
        a CUDA tensor (Hd, Wd, 3) float32 or (Hd, Wd, 4) float16 (RGBA16F)
        whose row stride is the pitch.  prev_pixel: float32, Hd * Wd * 2, the
        previous position of each display pixel in process_frame's prev_pixel
        convention at display size; or motion: float32 / float16 vectors with
        motion_scale, motion_at_pixel_centre and pixel_offset as prepare takes
        them.  blend_alpha: None = the configuration's taa_blend_alpha.  dst: a
        surface as resolve takes it (origin, flip_y, bgr, alpha), written in
        the same pass.  The context only names the device.  -> result."""
        a, s = self.display_taa_args(current, result, history, prev_pixel, motion, motion_scale,
                                     motion_at_pixel_centre, pixel_offset, blend_alpha, reset, dst, origin, flip_y,
                                     bgr, alpha)
        check(self.lib.bmfr_display_taa(self.handle, _stream(stream), C.byref(a), C.byref(s) if s is not None else None),
              "bmfr_display_taa")
        return result

    @property
    def region(self):
        """(x, y, width, height) of the image pixels this context's planes hold."""
        s = self.sizes
        return s.region_x, s.region_y, s.region_width, s.region_height

    def copy_state(self, name: str, dst: torch.Tensor, previous: bool = False, stream=None) -> torch.Tensor:
        ptr = getattr(self.state(previous), name)
        hip_memcpy_d2d(dst.data_ptr(), ptr, dst.numel() * dst.element_size(), stream)
        return dst


_hip = None


def hip_memcpy_d2d(dst: int, src: int, nbytes: int, stream=None) -> None:
    """hipMemcpyAsync device-to-device on the torch stream (torch's HIP runtime)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7")
        _hip.hipMemcpyAsync.restype = C.c_int
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    err = _hip.hipMemcpyAsync(dst, src, nbytes, 3, _stream(stream))  # 3 = hipMemcpyDeviceToDevice
    if err != 0:
        raise RuntimeError(f"hipMemcpyAsync failed: {err}")


def synth_camera(width: int, height: int, frame: int):
    """(column-major VP of `frame`, pixel offset of `frame`) of the synthetic sequence."""
    vp = (C.c_float * 16)()
    off = (C.c_float * 2)()
    _lib.load().bmfr_synth_camera(width, height, frame, vp, off)
    return list(vp), list(off)


def synth_frame_host(width: int, height: int, frame: int, seed: int = 0x424D4652, clean: bool = False):
    """Render synthetic frame `frame` on the CPU -> dict of float32 numpy (H, W, 3)."""
    import numpy as np
    out = {k: np.empty((height, width, 3), np.float32) for k in ("noisy", "normals", "positions", "albedo")}
    if clean:
        out["clean"] = np.empty((height, width, 3), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    check(_lib.load().bmfr_synth_frame_host(width, height, frame, seed, p(out["noisy"]), p(out["normals"]),
                                            p(out["positions"]), p(out["albedo"]),
                                            p(out["clean"]) if clean else None), "bmfr_synth_frame_host")
    return out


def synth_region_device(width: int, height: int, region, frame: int, seed: int = 0x424D4652, device: int = 0,
                        clean: bool = False, out=None, stream=None):
    """Render the region (x, y, w, h) of synthetic frame `frame` (a tiled
    context's inputs) -> dict of float32 tensors (h*w*3), row stride w."""
    x0, y0, w, h = region
    dev = torch.device("cuda", device)
    keys = ("noisy", "normals", "positions", "albedo") + (("clean",) if clean else ())
    if out is None:
        out = {k: torch.empty(h * w * 3, dtype=torch.float32, device=dev) for k in keys}
    check(_lib.load().bmfr_synth_region_device(width, height, x0, y0, w, h, frame, seed, _ptr(out["noisy"]),
                                               _ptr(out["normals"]), _ptr(out["positions"]),
                                               _ptr(out["albedo"]), _ptr(out.get("clean")),
                                               _stream(stream)), "bmfr_synth_region_device")
    return out


def synth_frame_device(width: int, height: int, frame: int, seed: int = 0x424D4652, device: int = 0,
                       clean: bool = False, out=None, stream=None):
    """Render synthetic frame `frame` on the GPU -> dict of float32 tensors (H*W*3)."""
    dev = torch.device("cuda", device)
    keys = ("noisy", "normals", "positions", "albedo") + (("clean",) if clean else ())
    if out is None:
        out = {k: torch.empty(height * width * 3, dtype=torch.float32, device=dev) for k in keys}
    check(_lib.load().bmfr_synth_frame_device(width, height, frame, seed, _ptr(out["noisy"]),
                                              _ptr(out["normals"]), _ptr(out["positions"]),
                                              _ptr(out["albedo"]), _ptr(out.get("clean")),
                                              _stream(stream)), "bmfr_synth_frame_device")
    return out
