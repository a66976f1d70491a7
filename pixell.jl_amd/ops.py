"""Device operators: the reference's batched evaluators and the reprojection, through the C ABI.

Names, argument meaning and `safe` keyword follow /root/reference/src/projections/car_proj.jl and
src/enmap_ops.jl.  Dispatch mirrors the reference's methods:

    pix2sky(m, pix2xN)            car_proj.jl:118-122   device, 2xN batch == torch tensor of shape (N, 2)
    pix2sky(m, ivec, jvec)        car_proj.jl:141-152   device, two N-vectors (broadcast form)
    pix2sky(m, i, j)              car_proj.jl:141-152   host scalar
    pix2sky(m, [i, j])            car_proj.jl:155-162   host scalar, length-2 vector
    sky2pix(m, sky2xN)            car_proj.jl:196-200   device
    sky2pix(m, ravec, decvec)     car_proj.jl:235-252   device
    sky2pix(m, ra, dec)           car_proj.jl:220-234   host scalar
    sky2pix(m, [ra, dec])         car_proj.jl:255-259   host scalar

`m` is an Enmap or a (shape, wcs) pair (enmap_ops.jl:60-66).  Every device path calls libpixell_hip.so;
nothing here computes on the CPU in its place.
"""
import ctypes as C
import math

import torch

from . import _lib, placement
from ._lib import FORM_DIV, FORM_RECIP, FORM_RECIP_AV, WRAP_NONE, WRAP_REWIND, WRAP_UNWIND
from .enmap import Enmap, _geom
from .wcs import (AbstractCARWCS, Gnomonic, pix2sky_scalar, pix2sky_tan_scalar, sky2pix_scalar,
                  sky2pix_tan_scalar)


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _dev_f64(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch tensor" % what)
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU: the MI355X path has no CPU fallback "
                           "(CPU arrays stay with the reference implementation)" % what)
    if t.dtype != torch.float64:
        raise TypeError("%s must be float64" % what)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    return t


def _dev_map(t: torch.Tensor, what: str) -> torch.Tensor:
    """Map storage may be Float64 or Float32 (coordinates are always Float64)."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.float32:
        if not t.is_cuda:
            raise RuntimeError("%s must live on the GPU: the MI355X path has no CPU fallback" % what)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % what)
        return t
    return _dev_f64(t, what)


def _ptr(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


def _is_scalar(x):
    return isinstance(x, (int, float))


def _wcs_ref(wcs):
    return C.byref(wcs.to_struct())


def _shape2(shape):
    return _lib.shape_arr((shape[0], shape[1]))


# ---- argument checks, each written once ---------------------------------------------------------------------------------
# The C ABI takes a pointer and a count and cannot see how long a buffer is: a tensor's extent is checked here, against what
# the kernel will touch, or nowhere.  Every entry below goes through these helpers, so a check one operator has, all have.

def _call(name, on, *args):
    """Call the library entry `name` on the device and the current stream of `on` (a tensor, or a plan: anything with a
    `.device`): the stream goes last, as in every entry that launches, and a non-zero status raises PixellHipError."""
    with torch.cuda.device(on.device):
        rc = getattr(_lib.load(), name)(*args, _stream(on))
    if rc != 0:                                      # every operator's hot path: the call into _lib.check only when it will raise
        _lib.check(rc)


def _no_f32(op, t, noun):
    """The operator's own refusal of Float32, where _dev_f64's TypeError would not say who takes what."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.float32:
        raise ValueError("%s takes Float64 %s" % (op, noun))


def _f64(t, what, op, noun=None):
    _no_f32(op, t, noun or what)
    return _dev_f64(t, what)


def _on(t, what, device):
    """`t` where it already passed its other checks, on the device the call runs on."""
    if t.device != device:
        raise ValueError("%s must be on %s" % (what, device))
    return t


def _coords(t, what, device=None, n=None):
    """An (N, 2) Float64 coordinate batch, of n points if n is given.  device: for the operators whose message names the device
    the batch belongs on; the others hand the batch to _on."""
    sky = _dev_f64(t, what)
    if sky.dim() != 2 or sky.shape[1] != 2 or (device is not None and sky.device != device) or (n is not None and sky.shape[0] != n):
        raise ValueError("coordinate batches are (N, 2) tensors (Julia 2xN)" + ("" if device is None else " on %s" % (device,)))
    return sky


def _vec_pair(a, b, name_a, name_b):
    """Two Float64 vectors of one shape on one device (the broadcast forms): the count passed on is a.numel()."""
    a, b = _dev_f64(a, name_a), _dev_f64(b, name_b)
    if a.shape != b.shape:
        raise ValueError("%s and %s must have the same shape" % (name_a, name_b))
    return a, _on(b, name_b, a.device)


def _ncomp(data: torch.Tensor) -> int:
    """The component count of ([nc,] ny, nx) data."""
    return data.shape[0] if data.dim() == 3 else 1


def _shape3(shape, nc):
    """The Julia-order triple (nx, ny, nc) the library takes."""
    return _lib.shape_arr((shape[0], shape[1], nc))


def _row_window(shape, src_rows, data=None):
    """(nx, ny), row0, nrows of the declination strip `src_rows` = (row0, nrows) of a map of Julia shape `shape` (the whole map for
    None), inside the map's rows.  data: the resident ([nc,] nrows, nx) tensor of a sampler, which must be exactly that strip."""
    nx, ny = int(shape[0]), int(shape[1])
    row0, nrows = (0, ny) if src_rows is None else (int(src_rows[0]), int(src_rows[1]))
    inside = row0 >= 0 and nrows >= 0 and row0 + nrows <= ny
    if data is not None and (not inside or data.shape[-2] != nrows or data.shape[-1] != nx):
        raise ValueError("the map's data %s is not rows [%d, %d) of a %d x %d map" % (tuple(data.shape), row0, row0 + nrows, nx, ny))
    if not inside:
        raise ValueError("rows [%d, %d) lie outside the map's %d rows" % (row0, row0 + nrows, ny))
    return (nx, ny), row0, nrows


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * 8 and b0 < a0 + a.numel() * 8


def _out_map(out, wcs, alloc, device, shapes=None, elems=None, f32=None, clear=(), clear_msg="out overlaps the input map",
             inplace=None):
    """The map an operator writes: `out` is None (then alloc() makes the tensor), an Enmap or a tensor.  Returns (dst, res): the
    Float64 tensor to write and the Enmap to return (`out` itself if it is one).  dst is on `device`; its shape is one of
    `shapes` (the first is the one named in the message), or it holds the elems = (nc, ny, nx) elements; it overlaps none of
    the tensors in `clear`, nor `inplace` unless it is exactly that tensor.  f32: the operator's own refusal of Float32."""
    if out is None:
        out = Enmap(alloc(), wcs)
    dst = out.data if isinstance(out, Enmap) else out
    if f32 is not None and isinstance(dst, torch.Tensor) and dst.dtype == torch.float32:
        raise ValueError(f32)
    dst = _dev_f64(dst, "out")
    if shapes is not None and (tuple(dst.shape) not in shapes or dst.device != device):
        raise ValueError("out must be a %s map on %s" % (shapes[0], device))
    if elems is not None and (dst.numel() != elems[0] * elems[1] * elems[2] or dst.device != device):
        raise ValueError("out must hold %d x %d x %d elements on %s" % (elems + (device,)))
    for t in clear:
        if _overlap(dst, t):
            raise ValueError(clear_msg)
    if inplace is not None and dst.data_ptr() != inplace.data_ptr() and _overlap(dst, inplace):
        raise ValueError(clear_msg)
    return dst, out if isinstance(out, Enmap) else Enmap(dst, wcs)


def _require_car(wcs):
    if not isinstance(wcs, AbstractCARWCS):
        raise TypeError("only CAR WCS (CarClenshawCurtis / CarFejer1) and Gnomonic are accelerated; "
                        "generic WCSTransform maps stay on the reference's wcslib path")


def _car_only(wcs, what):
    if isinstance(wcs, Gnomonic):
        raise ValueError("%s is CAR only" % what)
    _require_car(wcs)


def _iqu_map(m, what):
    if not isinstance(m.data, torch.Tensor) or m.data.dim() != 3 or m.data.shape[0] != 3:
        raise ValueError("%s takes a map of exactly three components (I, Q, U)" % what)


def _rcond_min(rcond_min) -> float:
    rmin = float(rcond_min)
    if not (0.0 < rmin <= 1.0):
        raise ValueError("rcond_min must lie in (0, 1], not %r" % (rcond_min,))
    return rmin


def _sample_vectors(what, d, w):
    """The (N,) samples `d` and weights `w` of a map-maker."""
    _f64(d, "d", what)
    _f64(w, "w", what)
    if d.dim() != 1 or tuple(w.shape) != tuple(d.shape) or w.device != d.device:
        raise ValueError("d and w must be (N,) tensors on one device")


# ---- pix2sky ------------------------------------------------------------------------------------

def pix2sky_(m, pixcoords, skycoords, safe=True):
    """pix2sky!(m, pixcoords, skycoords; safe) -- car_proj.jl:92-115.  Returns skycoords."""
    shape, wcs = _geom(m)
    _require_car(wcs)
    pix = _coords(pixcoords, "pixcoords")
    sky = _on(_coords(skycoords, "skycoords", n=pix.shape[0]), "skycoords", pix.device)
    _call("pxl_pix2sky_car_f64", pix, _wcs_ref(wcs), pix.shape[0], _ptr(pix), _ptr(sky), WRAP_UNWIND if safe else WRAP_NONE)
    return sky


def pix2sky(m, p1, p2=None, safe=True):
    shape, wcs = _geom(m)
    if isinstance(wcs, Gnomonic):
        return _pix2sky_tan(shape, wcs, p1, p2)
    _require_car(wcs)
    if p2 is None:
        if isinstance(p1, torch.Tensor):
            return pix2sky_(m, p1, torch.empty_like(p1), safe=safe)
        if len(p1) != 2:                       # @assert length(pixcoords) == 2, car_proj.jl:156
            raise AssertionError("length(pixcoords) == 2")
        # car_proj.jl:157: the inner scalar call does not forward `safe` (always rewinds);
        # the unwind! that follows is a no-op on one point.
        return list(pix2sky_scalar(shape, wcs, p1[0], p1[1], safe=True))
    if _is_scalar(p1) and _is_scalar(p2):
        return pix2sky_scalar(shape, wcs, p1, p2, safe=safe)
    ip, jp = _vec_pair(p1, p2, "ra_pixel", "dec_pixel")
    ra, dec = torch.empty_like(ip), torch.empty_like(jp)
    _call("pxl_pix2sky_car_soa_f64", ip, _wcs_ref(wcs), ip.numel(), _ptr(ip), _ptr(jp), _ptr(ra), _ptr(dec), int(bool(safe)))
    return ra, dec


def pix2sky_rewind(m, pixcoords):
    """2xN pix2sky with the per-element rewind of the scalar method (PXL_WRAP_REWIND)."""
    shape, wcs = _geom(m)
    _require_car(wcs)
    pix = _coords(pixcoords, "pixcoords")
    sky = torch.empty_like(pix)
    _call("pxl_pix2sky_car_f64", pix, _wcs_ref(wcs), pix.shape[0], _ptr(pix), _ptr(sky), WRAP_REWIND)
    return sky


# ---- rewind / unwind on device arrays (enmap_ops.jl:10-32) ----------------------------------------

def rewind_(angles: torch.Tensor, period=2 * 3.141592653589793, ref_angle=0.0):
    """rewind!(angles; period, ref_angle), elementwise, in place."""
    a = _dev_f64(angles, "angles")
    _call("pxl_rewind_f64", a, _ptr(a), a.numel(), float(period), float(ref_angle))
    return angles


def unwind_(angles: torch.Tensor, period=2 * 3.141592653589793, ref_angle=0.0):
    """unwind!(angles; dims=2, ...) for an (N, 2) coordinate batch, or along a 1-D vector; in place."""
    a = _dev_f64(angles, "angles")
    if a.dim() == 2 and a.shape[1] == 2:
        n, nrow = a.shape[0], 2
    elif a.dim() == 1:
        n, nrow = a.shape[0], 1
    else:
        raise ValueError("unwind_ takes an (N, 2) batch or a 1-D vector")
    _call("pxl_unwind_f64", a, _ptr(a), n, nrow, float(period), float(ref_angle))
    return angles


# ---- sky2pix ------------------------------------------------------------------------------------

def sky2pix_(m, skycoords, pixcoords, safe=True):
    """sky2pix!(m, skycoords, pixcoords; safe) -- car_proj.jl:165-193.  Returns pixcoords."""
    shape, wcs = _geom(m)
    _require_car(wcs)
    sky = _coords(skycoords, "skycoords")
    pix = _on(_coords(pixcoords, "pixcoords", n=sky.shape[0]), "pixcoords", sky.device)
    _call("pxl_sky2pix_car_f64", sky, _wcs_ref(wcs), _shape2(shape), sky.shape[0], _ptr(sky), _ptr(pix), int(bool(safe)), FORM_RECIP)
    return pix


def _sky2pix_soa(shape, wcs, ra, dec, safe, form):
    """The two-vector sky2pix of a CAR map in the arithmetic form `form`."""
    ra, dec = _vec_pair(ra, dec, "ra", "dec")
    ip, jp = torch.empty_like(ra), torch.empty_like(dec)
    _call("pxl_sky2pix_car_soa_f64", ra, _wcs_ref(wcs), _shape2(shape), ra.numel(), _ptr(ra), _ptr(dec), _ptr(ip), _ptr(jp),
          int(bool(safe)), form)
    return ip, jp


def sky2pix(m, p1, p2=None, safe=True):
    shape, wcs = _geom(m)
    if isinstance(wcs, Gnomonic):
        return _sky2pix_tan(shape, wcs, p1, p2)
    _require_car(wcs)
    if p2 is None:
        if isinstance(p1, torch.Tensor):
            return sky2pix_(m, p1, torch.empty_like(p1), safe=safe)
        if len(p1) != 2:                       # car_proj.jl:256
            raise AssertionError("length(skycoords) == 2")
        return list(sky2pix_scalar(shape, wcs, p1[0], p1[1], safe=safe))
    if _is_scalar(p1) and _is_scalar(p2):
        return sky2pix_scalar(shape, wcs, p1, p2, safe=safe)
    return _sky2pix_soa(shape, wcs, p1, p2, safe, FORM_RECIP_AV)


def sky2pix_broadcast(m, ra, dec, safe=True):
    """sky2pix.(Ref(m), ra, dec): the scalar (division) form of car_proj.jl:220-234 over two vectors."""
    shape, wcs = _geom(m)
    _require_car(wcs)
    return _sky2pix_soa(shape, wcs, ra, dec, safe, FORM_DIV)


# ---- Gnomonic -----------------------------------------------------------------------------------

def _pix2sky_tan(shape, wcs, p1, p2):
    if _is_scalar(p1) and _is_scalar(p2):
        return pix2sky_tan_scalar(shape, wcs, p1, p2)
    ip, jp = _vec_pair(p1, p2, "ra_pixel", "dec_pixel")
    ra, dec = torch.empty_like(ip), torch.empty_like(jp)
    _call("pxl_pix2sky_tan_f64", ip, _wcs_ref(wcs), ip.numel(), _ptr(ip), _ptr(jp), _ptr(ra), _ptr(dec))
    return ra, dec


def _sky2pix_tan(shape, wcs, p1, p2):
    if _is_scalar(p1) and _is_scalar(p2):
        return sky2pix_tan_scalar(shape, wcs, p1, p2)
    ra, dec = _vec_pair(p1, p2, "ra", "dec")
    ip, jp = torch.empty_like(ra), torch.empty_like(dec)
    _call("pxl_sky2pix_tan_f64", ra, _wcs_ref(wcs), ra.numel(), _ptr(ra), _ptr(dec), _ptr(ip), _ptr(jp))
    return ip, jp


# ---- whole-map writers --------------------------------------------------------------------------

def posmap(shape, wcs, device="cuda", row0=0, nrows=None, safe=True):
    """posmap(shape, wcs) -- enmap_ops.jl:190-203: (ra_map, dec_map) Enmaps of the pixel centres.
    row0/nrows select a declination strip (0-based rows) for sharded use."""
    nx, ny = int(shape[0]), int(shape[1])
    nrows = ny - row0 if nrows is None else nrows
    dev = torch.device(device)
    ra = torch.empty((nrows, nx), dtype=torch.float64, device=dev)
    dec = torch.empty((nrows, nx), dtype=torch.float64, device=dev)
    if isinstance(wcs, Gnomonic):
        _call("pxl_posmap_tan_f64", ra, _wcs_ref(wcs), _shape2(shape), row0, nrows, _ptr(ra), _ptr(dec))
    else:
        _require_car(wcs)
        _call("pxl_posmap_car_f64", ra, _wcs_ref(wcs), _shape2(shape), row0, nrows, _ptr(ra), _ptr(dec), int(bool(safe)))
    strip_wcs = wcs
    if (row0, nrows) != (0, ny):
        from .geometry import slice_geometry
        _, strip_wcs = slice_geometry((nx, ny), wcs, None, (row0 + 1, row0 + nrows))
    return Enmap(ra, strip_wcs), Enmap(dec, strip_wcs)


def pixareamap_(pixareas: Enmap):
    """pixareamap!(pixareas) -- enmap_ops.jl:124-138."""
    shape, wcs = pixareas.shape, pixareas.wcs
    _require_car(wcs)
    data = _dev_f64(pixareas.data, "pixareas")
    for plane in (data if data.dim() == 3 else (data,)):
        _call("pxl_pixareamap_car_f64", data, _wcs_ref(wcs), _shape2(shape), 0, shape[1], _ptr(plane))
    return pixareas


def pixareamap(m, wcs=None, device="cuda"):
    """pixareamap(m::Enmap) / pixareamap(shape, wcs) -- car_proj.jl:264-272."""
    if isinstance(m, Enmap):
        return pixareamap_(m.similar())
    shape = tuple(m)
    data = torch.empty(tuple(reversed(shape)), dtype=torch.float64, device=device)
    return pixareamap_(Enmap(data, wcs))


# ---- distance_transform (transform_distance.jl) ---------------------------------------------------

class ExactSeqSDT:
    """transform_distance.jl:10-18.  `epsfactor` is kept for the reference's signature; the device result is exact."""

    def __init__(self, epsfactor=1.0):
        self.epsfactor = float(epsfactor)


class ApproxSeqSDT:
    """transform_distance.jl:8."""


class BruteForceSDT:
    """transform_distance.jl:7."""


def distance_transform(dt, m: Enmap, out=None) -> Enmap:
    """distance_transform(dt, m) -- transform_distance.jl:55-78, :193-203, :322-344: for every pixel of the 2-D Float64 CAR
    map `m` (on the device) the angular distance in radians to the nearest pixel whose value is zero (-0.0 counts, NaN does
    not).  Returns an Enmap with m's WCS (into `out` if given).

    Every `dt` kind runs the same exact transform (pxl_distance_transform_car_f64, O(pixels) whatever the mask).
    BruteForceSDT and ExactSeqSDT define that value.  ApproxSeqSDT asks for less: the reference's own test only requires
    that it differ from the exact transform in under 20 % of the pixels, so the exact result is at least as good.
    Raises ValueError for a non-CAR WCS (the reference's PrecomputedSkyAngles assumes a separable grid), a 3-D map,
    an `out` overlapping the input, a map with no zero pixel (where the reference's acos throws DomainError), and a geometry
    the entry refuses: rows of more than 131072 pixels, more than 360 degrees of RA, a row beyond a pole, DEC not monotone."""
    if not isinstance(dt, (ExactSeqSDT, ApproxSeqSDT, BruteForceSDT)):
        raise TypeError("dt must be ExactSeqSDT(), ApproxSeqSDT() or BruteForceSDT()")
    if not isinstance(m, Enmap):
        raise TypeError("distance_transform takes an Enmap")
    if not isinstance(m.wcs, AbstractCARWCS):
        raise ValueError("distance_transform needs a CAR WCS: the transform assumes RA depends on the column alone and DEC "
                         "on the row alone (PrecomputedSkyAngles)")
    data = _dev_f64(m.data, "map data")
    if data.dim() != 2:
        raise ValueError("distance_transform takes a 2-D map, not %d-D" % data.dim())
    dst, res = _out_map(out, m.wcs, lambda: torch.empty_like(data), data.device, shapes=(tuple(data.shape),), clear=(data,))
    try:
        _call("pxl_distance_transform_car_f64", data, _wcs_ref(m.wcs), _shape2(m.shape), _ptr(data), _ptr(dst))
    except _lib.PixellHipError as e:
        if e.code != -22:
            raise
        raise ValueError(str(e)) from None       # PXL_EINVAL: the entry's refusal of the map's geometry, its reason in the text
    # +Inf only when the map has no zero pixel
    if dst.view(-1)[0].item() == float("inf"):
        raise ValueError("distance_transform: the map has no zero pixel (the reference raises DomainError from acos)")
    return res


# ---- reprojection -------------------------------------------------------------------------------

class _PlanHandle:
    """What the two plan classes share: the device a plan's tables live on and the lifetime of its library handle `_h`, which the
    entry named by `_destroy` frees."""
    _destroy = None

    def _open(self, device):
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._h = C.c_void_p()

    def _on_device(self, src, dst):
        if src.device != self.device or dst.device != self.device:
            raise ValueError("plan lives on %s" % (self.device,))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(_lib.load(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReprojectPlan(_PlanHandle):
    """Owns a pxl_reproject_plan (device coordinate tables).  src/dst windows describe declination
    strips of sharded maps (0-based row0, nrows); full maps by default."""

    _destroy = "pxl_reproject_plan_destroy"

    def __init__(self, shape_in, wcs_in, shape_out, wcs_out, src_rows=None, dst_rows=None, device="cuda"):
        _require_car(wcs_in)
        _require_car(wcs_out)
        self.shape_in = (int(shape_in[0]), int(shape_in[1]), int(shape_in[2]) if len(shape_in) > 2 else 1)
        self.shape_out = (int(shape_out[0]), int(shape_out[1]))
        self.wcs_in, self.wcs_out = wcs_in, wcs_out
        # the windows are the library's to refuse (pxl_reproject_plan_create), so they are not _row_window's
        self.src_rows = (0, self.shape_in[1]) if src_rows is None else (int(src_rows[0]), int(src_rows[1]))
        self.dst_rows = (0, self.shape_out[1]) if dst_rows is None else (int(dst_rows[0]), int(dst_rows[1]))
        self._open(device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pxl_reproject_plan_create(
                _wcs_ref(wcs_in), _lib.shape_arr(self.shape_in), self.src_rows[0], self.src_rows[1],
                _wcs_ref(wcs_out), _lib.shape_arr(self.shape_out), self.dst_rows[0], self.dst_rows[1],
                C.byref(self._h)))

    @property
    def ncomp(self):
        return self.shape_in[2]

    def src_tensor_shape(self):
        return (self.ncomp, self.src_rows[1], self.shape_in[0])

    def dst_tensor_shape(self):
        return (self.ncomp, self.dst_rows[1], self.shape_out[0])

    def set_variant(self, variant: int):
        _lib.check(_lib.load().pxl_reproject_plan_set_variant(self._h, int(variant)))

    def src_rows_needed(self):
        lo, hi = C.c_int64(), C.c_int64()
        _lib.check(_lib.load().pxl_reproject_plan_src_rows(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def rows_covered(self, have_lo, have_hi):
        lo, hi = C.c_int64(), C.c_int64()
        _lib.check(_lib.load().pxl_reproject_plan_rows_covered(self._h, have_lo, have_hi, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def _check(self, src, dst):
        src, dst = _dev_map(src, "src"), _dev_map(dst, "dst")
        if src.dtype != dst.dtype:
            raise TypeError("src and dst must have the same dtype (Float64 or Float32)")
        if src.numel() != self.ncomp * self.src_rows[1] * self.shape_in[0]:
            raise ValueError("src has %d elements, plan expects %s" % (src.numel(), (self.src_tensor_shape(),)))
        if dst.numel() != self.ncomp * self.dst_rows[1] * self.shape_out[0]:
            raise ValueError("dst has %d elements, plan expects %s" % (dst.numel(), (self.dst_tensor_shape(),)))
        self._on_device(src, dst)
        if src.data_ptr() == dst.data_ptr():
            raise ValueError("src and dst must not alias")
        return src, dst

    def execute(self, src, dst):
        src, dst = self._check(src, dst)
        _call("pxl_reproject_execute_f32" if src.dtype == torch.float32 else "pxl_reproject_execute", dst, self._h, _ptr(src), _ptr(dst))
        return dst

    def build_tables(self):
        _call("pxl_reproject_build_tables", self, self._h)

    def execute_rows(self, src, dst, r0, nr):
        src, dst = self._check(src, dst)
        _call("pxl_reproject_execute_rows_f32" if src.dtype == torch.float32 else "pxl_reproject_execute_rows", dst, self._h,
              _ptr(src), _ptr(dst), r0, nr)
        return dst


def _check_order(order):
    if order not in (1, 3):
        raise ValueError("order must be 1 (bilinear) or 3 (cubic B-spline), not %r" % (order,))


def _cubic_shape(shape, what):
    if int(shape[0]) < 4 or int(shape[1]) < 4:
        raise ValueError("%s: order=3 needs a map of at least 4 x 4 pixels" % what)


def _cubic_map(m: Enmap, what: str) -> torch.Tensor:
    """The limits of the order-3 path, checked on the host before any device work."""
    if isinstance(m.wcs, Gnomonic):
        raise ValueError("%s: order=3 is CAR only; a Gnomonic map is interpolated with order=1" % what)
    _require_car(m.wcs)
    if isinstance(m.data, torch.Tensor) and m.data.dtype == torch.float32:
        raise ValueError("%s: order=3 takes Float64 maps; a Float32 map is interpolated with order=1" % what)
    _cubic_shape(m.shape, what)
    return _dev_f64(m.data, "map data")


def _prefilter(what, entry, m, out):
    """spline_prefilter and its transpose: one pass of `entry` over every component of `m`."""
    if not isinstance(m, Enmap):
        raise TypeError("%s takes an Enmap" % what)
    data = _cubic_map(m, what)
    dst, res = _out_map(out, m.wcs, lambda: torch.empty_like(data), data.device, shapes=(tuple(data.shape),), clear=(data,))
    _call(entry, data, _wcs_ref(m.wcs), _shape3(m.shape, _ncomp(data)), _ptr(data), _ptr(dst))
    return res


def spline_prefilter(m: Enmap, out: Enmap = None) -> Enmap:
    """Cubic B-spline coefficients of every component of the Float64 CAR map `m` (pxl_spline_prefilter_car_f64):
    what `reproject(..., order=3, prefiltered=True)` and `sample(..., order=3, prefiltered=True)` evaluate.  Cyclic along RA on
    a full-circle map, mirrored at the other edges.  Returns an Enmap with m's WCS (into `out` if given; it may not overlap m)."""
    return _prefilter("spline_prefilter", "pxl_spline_prefilter_car_f64", m, out)


def _coeffs(m: Enmap, data: torch.Tensor, prefiltered) -> torch.Tensor:
    """The spline coefficients an order-3 evaluator reads: `data` itself if it already holds them, else spline_prefilter's pass
    into a temporary on data's stream."""
    if prefiltered:
        return data
    coeffs = torch.empty_like(data)                  # temporary: freed on return (the caching allocator orders it on the stream)
    _call("pxl_spline_prefilter_car_f64", data, _wcs_ref(m.wcs), _shape3(m.shape, _ncomp(data)), _ptr(data), _ptr(coeffs))
    return coeffs


def _reproject_cubic(m: Enmap, shape_out, wcs_out, out, plan, prefiltered) -> Enmap:
    nxo, nyo = shape_out
    if isinstance(wcs_out, Gnomonic):
        raise ValueError("reproject: order=3 is CAR only; a Gnomonic output is interpolated with order=1")
    _require_car(wcs_out)
    if plan is not None:
        if not isinstance(plan, ReprojectPlan):
            raise TypeError("a CAR -> CAR reprojection takes a ReprojectPlan")
        if plan.src_rows != (0, plan.shape_in[1]) or plan.dst_rows != (0, plan.shape_out[1]):
            raise ValueError("reproject: order=3 works on full maps; this plan was built over a row window "
                             "(a strip would need a 34-row halo for the prefilter)")
        if plan.shape_in[:2] != (int(m.shape[0]), int(m.shape[1])) or plan.shape_out != (nxo, nyo):
            raise ValueError("plan was made for %s -> %s" % (plan.shape_in[:2], plan.shape_out))
    data = _cubic_map(m, "reproject")
    nc = _ncomp(data)
    oshape = (nyo, nxo) if data.dim() == 2 else (nc, nyo, nxo)
    dst, res = _out_map(out, wcs_out, lambda: placement.empty_map(oshape, dtype=data.dtype, device=m.device)[0], data.device,
                        elems=(nc, nyo, nxo), clear=(data,))
    coeffs = _coeffs(m, data, prefiltered)
    _call("pxl_reproject_car_cubic_f64", data, _wcs_ref(m.wcs), _shape3(m.shape, nc), _ptr(coeffs), _wcs_ref(wcs_out),
          _shape2((nxo, nyo)), _ptr(dst))
    return res


def sample(m: Enmap, skycoords: torch.Tensor, order=1, prefiltered=False) -> torch.Tensor:
    """Sample every component of `m` at a 2xN batch of (ra, dec); returns a (nc, N) tensor.  order=1 is sample_bilinear;
    order=3 evaluates the cubic B-spline of DESIGN 4.9 at sky2pix!(safe=true) of each point (pxl_sample_car_cubic_f64) after
    prefiltering `m` into a temporary, or straight from `m` when prefiltered=True says it already holds spline_prefilter's
    coefficients.  Points outside the map's pixel edges give 0."""
    _check_order(order)
    if order == 1:
        if prefiltered:
            raise ValueError("prefiltered=True only means something with order=3")
        return sample_bilinear(m, skycoords)
    data = _cubic_map(m, "sample")
    sky = _on(_coords(skycoords, "skycoords"), "skycoords", data.device)
    nc = _ncomp(data)
    out = torch.empty((nc, sky.shape[0]), dtype=torch.float64, device=sky.device)
    coeffs = _coeffs(m, data, prefiltered)
    _call("pxl_sample_car_cubic_f64", sky, _wcs_ref(m.wcs), _shape3(m.shape, nc), _ptr(coeffs), sky.shape[0], _ptr(sky), _ptr(out))
    return out


def reproject(m: Enmap, shape_out, wcs_out, out: Enmap = None, plan: ReprojectPlan = None, order=1, prefiltered=False) -> Enmap:
    """CAR -> CAR reprojection of every component of `m` onto (shape_out, wcs_out).  order=1 (the default): bilinear.
    Not in the reference; composes posmap(out) o sky2pix(in) o 2x2 gather + lerp.
    order=3: cubic B-spline at the same source positions: `m` is prefiltered into a temporary,
    or taken as spline_prefilter's coefficients when prefiltered=True.  Float64 CAR full maps only."""
    _check_order(order)
    nxo, nyo = int(shape_out[0]), int(shape_out[1])
    if order == 3:
        return _reproject_cubic(m, (nxo, nyo), wcs_out, out, plan, prefiltered)
    if prefiltered:
        raise ValueError("prefiltered=True only means something with order=3")
    if isinstance(m.wcs, Gnomonic) or isinstance(wcs_out, Gnomonic):
        return _reproject_generic(m, (nxo, nyo), wcs_out, out, plan)
    if plan is None:
        plan = ReprojectPlan(m.shape, m.wcs, shape_out, wcs_out, device=m.device)
    if out is None:
        # the library's allocation policy for map-sized outputs (placement.empty_map): by default a destination of 3 GiB or more
        # is placed across a boundary between two memory classes of the HBM -- no head-room is kept -- because the kernel's
        # eight write fronts store 15 % faster there; PXL_ALLOC_POLICY=plain or pj.set_allocation_policy("plain")
        # turn that into torch.empty.  Allocate once and pass `out=` (and `plan=`) when reprojecting repeatedly.
        oshape = (nyo, nxo) if m.data.dim() == 2 else (m.data.shape[0], nyo, nxo)
        data, _info = placement.empty_map(oshape, dtype=m.data.dtype, device=m.device)
        out = Enmap(data, wcs_out)
    plan.execute(m.data, out.data)                   # the plan checks both tensors (Float32 storage included)
    return out


def _proj_code(w):
    if not isinstance(w, (AbstractCARWCS, Gnomonic)):
        raise TypeError("generic reprojection handles CAR and Gnomonic WCS only")
    return 1 if isinstance(w, Gnomonic) else 0   # PXL_PROJ_TAN / PXL_PROJ_CAR


class GenericReprojectPlan(_PlanHandle):
    """Owns a pxl_generic_plan: the coordinate lattice of a CAR <-> Gnomonic reprojection (42 exact evaluations and 12 check
    points per 128 x 32 output tile) and the list of tiles that are evaluated per pixel.  What ReprojectPlan's tables are to
    the separable CAR -> CAR path: make it once per pair of geometries, execute it on as many maps as there are --
    `pj.reproject(m, shape_out, wcs_out, out=out, plan=plan)`.  Same results as the one-shot call, bit for bit."""

    _destroy = "pxl_generic_plan_destroy"

    def __init__(self, shape_in, wcs_in, shape_out, wcs_out, device="cuda"):
        self.shape_in = (int(shape_in[0]), int(shape_in[1]))
        self.shape_out = (int(shape_out[0]), int(shape_out[1]))
        self.wcs_in, self.wcs_out = wcs_in, wcs_out
        self._open(device)
        with torch.cuda.device(self.device):         # the stream is not the last argument here
            s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(_lib.load().pxl_generic_plan_create(
                _wcs_ref(wcs_in), _proj_code(wcs_in), _shape2(self.shape_in),
                _wcs_ref(wcs_out), _proj_code(wcs_out), _shape2(self.shape_out), s, C.byref(self._h)))

    def tiles(self):
        """(tiles evaluated per pixel, all tiles)"""
        a, b = C.c_int64(), C.c_int64()
        _lib.check(_lib.load().pxl_generic_plan_tiles(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def execute(self, src, dst):
        src, dst = _dev_f64(src, "src"), _dev_f64(dst, "dst")
        nx, ny = self.shape_in
        if src.dim() not in (2, 3) or tuple(src.shape[-2:]) != (ny, nx):
            raise ValueError("src has shape %s, plan expects (..., %d, %d)" % (tuple(src.shape), ny, nx))
        nc = _ncomp(src)
        if dst.numel() != nc * self.shape_out[0] * self.shape_out[1]:
            raise ValueError("dst has %d elements, plan expects %d x %d x %d" % (dst.numel(), nc, self.shape_out[1], self.shape_out[0]))
        self._on_device(src, dst)
        if src.data_ptr() == dst.data_ptr():
            raise ValueError("src and dst must not alias")
        _call("pxl_generic_plan_execute", dst, self._h, nc, _ptr(src), _ptr(dst))
        return dst


def _reproject_generic(m: Enmap, shape_out, wcs_out, out=None, plan=None) -> Enmap:
    """CAR <-> Gnomonic (non-separable) bilinear reprojection: pxl_reproject_generic_bilinear_f64, or a GenericReprojectPlan."""
    data = _dev_f64(m.data, "map data")
    code = _proj_code
    code(m.wcs), code(wcs_out)
    nc = _ncomp(data)
    nxo, nyo = shape_out

    def alloc():
        return torch.empty((nyo, nxo) if data.dim() == 2 else (nc, nyo, nxo), dtype=torch.float64, device=data.device)
    if plan is not None:
        if not isinstance(plan, GenericReprojectPlan):
            raise TypeError("a CAR <-> Gnomonic reprojection takes a GenericReprojectPlan")
        if plan.shape_in != (int(m.shape[0]), int(m.shape[1])) or plan.shape_out != (nxo, nyo):
            raise ValueError("plan was made for %s -> %s" % (plan.shape_in, plan.shape_out))
        if out is None:
            out = Enmap(alloc(), wcs_out)
        plan.execute(data, out.data)                 # the plan checks `out`, under its own messages
        return out
    dst, res = _out_map(out, wcs_out, alloc, data.device, elems=(nc, nyo, nxo), clear=(data,))
    _call("pxl_reproject_generic_bilinear_f64", data, _wcs_ref(m.wcs), code(m.wcs), _shape3(m.shape, nc), _ptr(data),
          _wcs_ref(wcs_out), code(wcs_out), _shape2(shape_out), _ptr(dst))
    return res


class SamplePairs:
    """Row-pair copy of a map for scattered sampling (pxl_sample_build_pairs_*): 8/3 of the footprint, ONE random
    64-byte sector per point instead of 2.25.  Build once per map, pass to sample_bilinear(..., pairs=...)."""

    def __init__(self, m: Enmap, src_rows=None, full_shape=None, out: torch.Tensor = None):
        data = _dev_map(m.data, "map data")
        _require_car(m.wcs)
        self.wcs = m.wcs
        self.shape = tuple(m.shape if full_shape is None else full_shape)
        self.nc = _ncomp(data)
        # the window is the library's to refuse (pxl_sample_pairs_elems), so it is not _row_window's
        self.src_rows = (0, self.shape[1]) if src_rows is None else (int(src_rows[0]), int(src_rows[1]))
        self.dtype = data.dtype
        n = _lib.load().pxl_sample_pairs_elems(_shape3(self.shape, self.nc), self.src_rows[1])
        if n < 0:
            raise _lib.PixellHipError(-22, _lib.last_error())
        self._resident(data)
        self.data = out if out is not None else torch.empty(n, dtype=data.dtype, device=data.device)
        if self.data.numel() != n or self.data.dtype != data.dtype or not self.data.is_contiguous():
            raise ValueError("pair buffer must hold %d contiguous %s elements" % (n, data.dtype))
        self.rebuild(data)

    def _resident(self, data):
        if data.numel() != self.nc * self.src_rows[1] * self.shape[0]:
            raise ValueError("map data does not match the resident window")

    def rebuild(self, data: torch.Tensor):
        """Re-derive the pair copy after the map changed (one streaming pass)."""
        data = _dev_map(data, "map data")
        self._resident(data)
        if data.dtype != self.dtype:
            raise ValueError("map data must be %s, like the pair buffer" % (self.dtype,))
        _on(data, "map data", self.data.device)
        _call("pxl_sample_build_pairs_f32" if data.dtype == torch.float32 else "pxl_sample_build_pairs_f64", data,
              _shape3(self.shape, self.nc), _ptr(data), self.src_rows[1], _ptr(self.data))
        return self


def _sample_rows(what, entry, m, skycoords, src_rows, full_shape, pol=False, resp=None, f32_first=False):
    """The map samplers of orders 0 and 1, scalar and polarised (pol: an IQU map and its (N, 2) responses, one sample per
    point): the Enmap, the CAR and the Float64 rules, the coordinates, the responses, the row window, the output and the call of
    `entry`.  what=None is sample_bilinear, which also takes Float32 maps and words its refusals as the oldest operators do;
    f32_first: the order-0 operators refuse every Float32 argument before they look at anything else of a tensor."""
    if what is None:
        data = _dev_map(m.data, "map data")
        _require_car(m.wcs)
        sky = _on(_coords(skycoords, "skycoords"), "skycoords", data.device)
        entry = entry.replace("_f64", "_f32") if data.dtype == torch.float32 else entry
    else:
        if not isinstance(m, Enmap):
            raise TypeError("%s takes an Enmap" % what)
        if pol:
            _iqu_map(m, what)
        _car_only(m.wcs, what)
        if f32_first:
            for t, noun in ((m.data, "maps"), (skycoords, "skycoords")) + (((resp, "resp"),) if pol else ()):
                _no_f32(what, t, noun)
        data = _f64(m.data, "map data", what, "maps")
        _no_f32(what, skycoords, "skycoords")
        sky = _coords(skycoords, "skycoords", data.device)
    r = (_ptr(_resp_arg(what, resp, sky)),) if pol else ()
    shape, row0, nrows = _row_window(m.shape if full_shape is None else full_shape, src_rows, data)
    nc = _ncomp(data)
    out = torch.empty((sky.shape[0],) if pol else (nc, sky.shape[0]), dtype=data.dtype, device=sky.device)
    _call(entry, sky, _wcs_ref(m.wcs), _shape3(shape, nc), _ptr(data), row0, nrows, sky.shape[0], _ptr(sky), *r, _ptr(out))
    return out


def sample_bilinear(m: Enmap, skycoords: torch.Tensor, src_rows=None, full_shape=None, pairs: SamplePairs = None) -> torch.Tensor:
    """Bilinear sample of every component of `m` at a 2xN batch of (ra, dec): fused
    sky2pix!(safe=true) [car_proj.jl:165-193] + 2x2 gather.  Returns a (nc, N) tensor.
    src_rows/full_shape describe `m.data` as a declination strip of a larger map.  pairs: a SamplePairs copy of
    the same map (then `m` may be None): same result, fewer random memory sectors per point."""
    if pairs is not None:
        sky = _on(_coords(skycoords, "skycoords"), "skycoords", pairs.data.device)
        out = torch.empty((pairs.nc, sky.shape[0]), dtype=pairs.dtype, device=sky.device)
        _call("pxl_sample_car_bilinear_pairs_f32" if pairs.dtype == torch.float32 else "pxl_sample_car_bilinear_pairs_f64", sky,
              _wcs_ref(pairs.wcs), _shape3(pairs.shape, pairs.nc), _ptr(pairs.data), pairs.src_rows[0], pairs.src_rows[1],
              sky.shape[0], _ptr(sky), _ptr(out))
        return out
    return _sample_rows(None, "pxl_sample_car_bilinear_f64", m, skycoords, src_rows, full_shape)


def _scatter_args(what, vals, skycoords, shape, wcs, out, src_rows=None, full_shape=None, planes=None):
    """The argument checks the scatter entries share, in scatter_bilinear's order.  Returns (v, sky, nc, dst, res, shape, row0,
    nrows): the device tensors, the component count, the (.., nrows, nx) tensor accumulated into, what the caller returns (`out`,
    or a fresh Enmap of zeros), the map's (nx, ny) and the row window.  planes (the polarised scatters): vals is one (N,) value
    per point and the map has that many planes."""
    _car_only(wcs, what)
    _no_f32(what, vals, "vals")
    _no_f32(what, skycoords, "skycoords")
    v = _dev_f64(vals, "vals")
    sky = _coords(skycoords, "skycoords")
    if v.dim() not in (1, 2) or v.shape[-1] != sky.shape[0] or v.device != sky.device:
        raise ValueError("vals must be (nc, N) or (N,) on %s with N = %d" % (sky.device, sky.shape[0]))
    if planes is not None and v.dim() != 1:
        raise ValueError("%s takes one value per point: vals is (N,)" % what)
    nc = v.shape[0] if v.dim() == 2 else 1
    if nc < 1:
        raise ValueError("vals needs at least one component")
    nc = nc if planes is None else planes
    shape, row0, nrows = _row_window(shape if full_shape is None else full_shape, src_rows)
    oshape = (nrows, shape[0]) if v.dim() == 1 and planes is None else (nc, nrows, shape[0])
    dst, res = _out_map(out, wcs, lambda: torch.zeros(oshape, dtype=torch.float64, device=sky.device), sky.device,
                        shapes=(oshape, (nc, nrows, shape[0])), f32="%s accumulates into Float64 maps" % what, clear=(v, sky),
                        clear_msg="out overlaps vals or skycoords")
    return v, sky, nc, dst, res, shape, row0, nrows


def _scatter_rows(what, entry, vals, skycoords, shape, wcs, out, src_rows, full_shape) -> Enmap:
    """scatter_bilinear and scatter_nearest: _scatter_args, then `entry` over the row window."""
    v, sky, nc, dst, res, shape, row0, nrows = _scatter_args(what, vals, skycoords, shape, wcs, out, src_rows, full_shape)
    _call(entry, sky, _wcs_ref(wcs), _shape3(shape, nc), _ptr(dst), row0, nrows, sky.shape[0], _ptr(sky), _ptr(v))
    return res


def scatter_bilinear(vals: torch.Tensor, skycoords: torch.Tensor, shape, wcs, out=None, src_rows=None, full_shape=None) -> Enmap:
    """The transpose of sample_bilinear (pxl_scatter_car_bilinear_f64): add `vals` at a 2xN batch of (ra, dec)
    into a Float64 CAR map, every point spread over its 2x2 cell with the sampler's own weights -- P^T d next to
    sample_bilinear's P m, or a hit-count map for vals = 1.  vals is (nc, N) or (N,); skycoords is (N, 2).  out=None
    allocates zeros of (nc, ny, nx), or (ny, nx) for 1-D vals; a given `out` (Enmap or tensor) is ACCUMULATED into and
    returned.  src_rows/full_shape describe `out` as a declination strip (row0, nrows) of a larger map, as for
    sample_bilinear.  The cell, seam and window rules are the sampler's bit for bit; a tap the sampler reads as 0 is dropped,
    a point whose position is not finite adds nothing, a NaN value makes its four taps NaN.
    The adds are hardware FP64 atomics: the order of the additions into one pixel is unspecified, so two calls on the same
    inputs may differ in the last bits wherever a pixel receives more than one non-zero term.  Pixels that receive nothing
    keep their bits.  Float64 and CAR only; `out` may not overlap vals or skycoords."""
    return _scatter_rows("scatter_bilinear", "pxl_scatter_car_bilinear_f64", vals, skycoords, shape, wcs, out, src_rows, full_shape)


def scatter_cubic(vals: torch.Tensor, skycoords: torch.Tensor, shape, wcs, out=None) -> Enmap:
    """E^T, the transpose of sample(order=3, prefiltered=True) (pxl_scatter_car_cubic_f64): add `vals` at a 2xN
    batch of (ra, dec) into a Float64 CAR map, every point spread over the sixteen taps the order-3 sampler reads, with its
    own weights and folded tap indices bit for bit (taps that fold onto one pixel next to a mirrored edge each add).
    Arguments and `out` as for scatter_bilinear, full maps only: `out` is ACCUMULATED into.  A point outside the map's pixel
    edges, or whose position is not finite, adds nothing; a NaN value makes its sixteen taps NaN.  The adds are hardware
    FP64 atomics, with scatter_bilinear's clause on the last bits.  The transpose of sample(order=3) itself is
    spline_prefilter_transpose of this map (what scatter(order=3) returns), not spline_prefilter of it."""
    _cubic_shape(shape, "scatter_cubic")
    v, sky, nc, dst, res, shape, _row0, _nrows = _scatter_args("scatter_cubic", vals, skycoords, shape, wcs, out)
    _call("pxl_scatter_car_cubic_f64", sky, _wcs_ref(wcs), _shape3(shape, nc), _ptr(dst), sky.shape[0], _ptr(sky), _ptr(v))
    return res


def spline_prefilter_transpose(g: Enmap, out: Enmap = None) -> Enmap:
    """F^T, the transpose of spline_prefilter (pxl_spline_prefilter_transpose_car_f64), of every component of the
    Float64 CAR map `g`: the prefilter's recursion between a doubling and a halving of the two edge lines of every mirrored
    axis (DEC always, RA unless the map is full-circle); RA first, then DEC.  Applied to scatter_cubic's map it gives P^T d for
    sample(order=3)'s P.  Returns an Enmap with g's WCS (into `out` if given; it may not overlap g)."""
    return _prefilter("spline_prefilter_transpose", "pxl_spline_prefilter_transpose_car_f64", g, out)


def scatter(vals: torch.Tensor, skycoords: torch.Tensor, shape, wcs, order=1, out=None, prefiltered=False) -> Enmap:
    """P^T d for sample(order=...)'s P: add `vals` at a 2xN batch of (ra, dec) into a Float64 CAR map.  order=1 is
    scatter_bilinear.  order=3 is F^T E^T d: scatter_cubic into a map of zeros, then spline_prefilter_transpose;
    a given `out` has the result added to it (a torch add: F^T cannot be accumulated through).  order=3 with
    prefiltered=True is E^T alone, scatter_cubic accumulating into `out`: the transpose of sample(order=3,
    prefiltered=True), and the way to gather many batches before one spline_prefilter_transpose."""
    _check_order(order)
    if order == 1:
        if prefiltered:
            raise ValueError("prefiltered=True only means something with order=3")
        return scatter_bilinear(vals, skycoords, shape, wcs, out=out)
    if prefiltered:
        return scatter_cubic(vals, skycoords, shape, wcs, out=out)
    if out is None:
        return spline_prefilter_transpose(scatter_cubic(vals, skycoords, shape, wcs))
    # every check of `out` before the first launch: it is what scatter_cubic would be given
    _cubic_shape(shape, "scatter")
    _v, _sky, _nc, dst, res, _shape, _row0, _nrows = _scatter_args("scatter", vals, skycoords, shape, wcs, out)
    g = scatter_cubic(vals, skycoords, shape, wcs)
    dst += spline_prefilter_transpose(g).data.view(dst.shape)
    return res


# ---- the polarised pointing matrix -------------------------------------------------------------------------

def _resp_arg(what, resp, sky):
    _no_f32(what, resp, "resp")
    r = _dev_f64(resp, "resp")
    if r.dim() != 2 or tuple(r.shape) != tuple(sky.shape) or r.device != sky.device:
        raise ValueError("resp must be (N, 2) pairs (q, u) on %s with N = %d" % (sky.device, sky.shape[0]))
    return r


def _pol_order(what, order, prefiltered, src_rows, full_shape):
    _check_order(order)
    if order == 1 and prefiltered:
        raise ValueError("prefiltered=True only means something with order=3")
    if order == 3 and (src_rows is not None or full_shape is not None):
        raise ValueError("%s: src_rows/full_shape are order=1 only; order=3 works on full maps" % what)


def sample_pol(m: Enmap, skycoords: torch.Tensor, resp: torch.Tensor, order=1, prefiltered=False, src_rows=None,
               full_shape=None) -> torch.Tensor:
    """P_pol m: the detector samples d = I + q Q + u U of the Float64 IQU CAR map `m` (exactly three components) at a 2xN
    batch of (ra, dec), in one pass (pxl_sample_car_pol_bilinear_f64 / pxl_sample_car_pol_cubic_f64).  `resp`
    is (N, 2) like skycoords: the pairs (q_k, u_k) = gamma (cos 2 psi, sin 2 psi), formed by the caller.  Returns (N,):
    out[k] = (s_I + q_k s_Q) + u_k s_U with s = sample(m, skycoords, order, prefiltered) (order 1: sample_bilinear with the
    same src_rows/full_shape), bit for bit, left to right without fma.  order, prefiltered as for sample; src_rows/full_shape
    (order 1 only) as for sample_bilinear.  Q and U are three independent scalar planes: no spin-2 sign flip is applied at
    the DEC mirror or across a pole."""
    _pol_order("sample_pol", order, prefiltered, src_rows, full_shape)
    if order == 1:
        return _sample_rows("sample_pol", "pxl_sample_car_pol_bilinear_f64", m, skycoords, src_rows, full_shape, pol=True, resp=resp)
    if not isinstance(m, Enmap):
        raise TypeError("sample_pol takes an Enmap")
    _iqu_map(m, "sample_pol")
    data = _cubic_map(m, "sample_pol")
    _no_f32("sample_pol", skycoords, "skycoords")
    sky = _coords(skycoords, "skycoords", data.device)
    r = _resp_arg("sample_pol", resp, sky)
    shape, _row0, _nrows = _row_window(m.shape, None, data)
    out = torch.empty((sky.shape[0],), dtype=torch.float64, device=sky.device)
    coeffs = _coeffs(m, data, prefiltered)
    _call("pxl_sample_car_pol_cubic_f64", sky, _wcs_ref(m.wcs), _shape3(shape, 3), _ptr(coeffs), sky.shape[0], _ptr(sky), _ptr(r), _ptr(out))
    return out


def _scatter_pol(what, mode, vals, skycoords, resp, shape, wcs, order, out, prefiltered, src_rows, full_shape) -> Enmap:
    """The polarised scatters of every order.  order 0 comes from the *_nearest operators alone: whoever takes an order= argument
    has put it through _pol_order, which knows 1 and 3."""
    if order == 0:
        _car_only(wcs, what)
        _no_f32(what, resp, "resp")
    if order == 3:
        _cubic_shape(shape, what)
    v, sky, _nc, dst, res, shp2, row0, nrows = _scatter_args(what, vals, skycoords, shape, wcs, out, src_rows, full_shape,
                                                             planes=6 if mode else 3)
    r = _resp_arg(what, resp, sky)
    if _overlap(dst, r):
        raise ValueError("out overlaps resp")
    shp = _shape3(shp2, 3)
    if order != 3:
        _call("pxl_scatter_car_pol_bilinear_f64" if order == 1 else "pxl_scatter_car_pol_nearest_f64", sky, _wcs_ref(wcs), shp,
              _ptr(dst), row0, nrows, sky.shape[0], _ptr(sky), _ptr(r), _ptr(v), mode)
        return res
    g = dst if prefiltered or out is None else torch.zeros_like(dst)
    _call("pxl_scatter_car_pol_cubic_f64", sky, _wcs_ref(wcs), shp, _ptr(g), sky.shape[0], _ptr(sky), _ptr(r), _ptr(v), mode)
    if prefiltered:
        return res
    ft = spline_prefilter_transpose(Enmap(g, wcs))
    if out is None:
        return ft
    dst += ft.data                                   # F^T cannot be accumulated through: a torch add, as scatter(order=3) does
    return res


def scatter_pol(vals: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, shape, wcs, order=1, out=None, prefiltered=False,
                src_rows=None, full_shape=None) -> Enmap:
    """P_pol^T d, the transpose of sample_pol: add the (N,) values `vals` at a 2xN batch of (ra, dec) into a Float64 IQU CAR
    map (3, ny, nx) in one pass (pxl_scatter_car_pol_bilinear_f64 / pxl_scatter_car_pol_cubic_f64).  With
    v = vals[k] and (q, u) = resp[k], plane I takes v, plane Q takes q v, plane U takes u v, each exactly as
    scatter(order=...) adds vals[c][k]: same taps, weights, seam, fold, domain, window and live rules, zero-weight taps
    included, the same hardware FP64 atomics with the same clause on the last bits.  out, order, prefiltered as for scatter
    (order 3: E^T into zeros, then spline_prefilter_transpose, a given `out` added to with a torch add; prefiltered=True
    accumulates E^T straight into `out`); src_rows/full_shape (order 1 only) as for scatter_bilinear.  Q and U are three
    independent scalar planes: no spin-2 sign flip is applied at the DEC mirror or across a pole.  `out` may not overlap
    vals, skycoords or resp."""
    _pol_order("scatter_pol", order, prefiltered, src_rows, full_shape)
    return _scatter_pol("scatter_pol", 0, vals, skycoords, resp, shape, wcs, order, out, prefiltered, src_rows, full_shape)


def scatter_pol_weights(w: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, shape, wcs, order=1, out=None,
                        prefiltered=False, src_rows=None, full_shape=None) -> Enmap:
    """The six independent planes II, IQ, IU, QQ, QU, UU of P_pol^T W P_pol's pixel blocks, (6, ny, nx): scatter_pol's adds with
    the sample weight w[k] times 1, q, u, q(q w), q(u w), u(u w) -- P^T applied to the six products, the block preconditioner
    and hit map of a polarised map-maker.  Arguments as for scatter_pol."""
    _pol_order("scatter_pol_weights", order, prefiltered, src_rows, full_shape)
    return _scatter_pol("scatter_pol_weights", 1, w, skycoords, resp, shape, wcs, order, out, prefiltered, src_rows, full_shape)


# ---- the per-pixel IQU block solve; the binned polarised map on top of it is mapmaker.py --------------------

def _polsolve_args(what, vec, vec_name, weights, out):
    """The argument checks pol_block_solve and pol_block_apply share.  Returns (x, w, dst, res): the (3, ny, nx) input, the
    (6, ny, nx) weights, the tensor written (x itself for an in-place call) and what the caller returns."""
    planes = []
    for m, name, np_ in ((vec, vec_name, 3), (weights, "weights", 6)):
        if not isinstance(m, Enmap):
            raise TypeError("%s: %s must be an Enmap" % (what, name))
        _car_only(m.wcs, what)
        t = _f64(m.data, name, what)
        if t.dim() != 3 or t.shape[0] != np_:
            raise ValueError("%s: %s must hold exactly %d planes, (%d, ny, nx)" % (what, name, np_, np_))
        planes.append(t)
    x, w = planes
    if tuple(w.shape[1:]) != tuple(x.shape[1:]) or w.device != x.device:
        raise ValueError("%s: weights must be a (6, %d, %d) map on %s" % (what, x.shape[1], x.shape[2], x.device))
    dst, res = _out_map(out, vec.wcs, lambda: torch.empty_like(x), x.device, shapes=(tuple(x.shape),),
                        f32="%s writes Float64 maps" % what, clear=(w,), inplace=x,
                        clear_msg="out overlaps weights, or %s other than exactly (out=%s works in place)" % (vec_name, vec_name))
    return x, w, dst, res


def pol_block_solve(rhs: Enmap, weights: Enmap, rcond_min=1e-3, out=None, return_rcond=False):
    """Solve the symmetric 3 x 3 system of every pixel (pxl_pol_block_solve_f64): `weights` is the (6, ny, nx) map
    II, IQ, IU, QQ, QU, UU that scatter_pol_weights accumulates, `rhs` the (3, ny, nx) map scatter_pol accumulates, both Float64
    CAR Enmaps on one device.  Returns the (3, ny, nx) solution, and with return_rcond=True also the (ny, nx) conditioning map.
    LDL^T with diagonal pivoting, defined to the bit in include/pixell_hip.h: with p1 >= p2, p3 the pivots, rc = min(p2, p3) / p1
    lies between the block's lambda_min / lambda_max and a small multiple of it.  A pixel is solved when p1 > 0, p2 / p1 and
    p3 / p1 are at least rcond_min, and its right-hand side is finite; every other pixel -- no hits, fewer than three hits, one
    polarisation angle, NaN or Inf anywhere -- is exactly +0.0 in all three planes, and its rcond is the computed rc if that is
    positive, else +0.0.  rcond_min lies in (0, 1].  out=rhs solves in place; any other `out` may not overlap rhs or weights."""
    x, w, dst, res = _polsolve_args("pol_block_solve", rhs, "rhs", weights, out)
    rmin = _rcond_min(rcond_min)
    rc = torch.empty(tuple(x.shape[1:]), dtype=torch.float64, device=x.device) if return_rcond else None
    _call("pxl_pol_block_solve_f64", x, _ptr(w), _ptr(x), _ptr(dst), _ptr(rc) if return_rcond else None, x.shape[1] * x.shape[2], rmin)
    return (res, Enmap(rc, rhs.wcs)) if return_rcond else res


def pol_block_apply(x: Enmap, weights: Enmap, out=None) -> Enmap:
    """The block product of every pixel (pxl_pol_block_apply_f64): out = A x with A the symmetric 3 x 3 block the
    six planes of `weights` hold, each row (m0 x0 + m1 x1) + m2 x2 left to right without fma -- the diagonal-block part of
    P^T W P, and the inverse of pol_block_solve on solved pixels.  Arguments as for pol_block_solve; out=x works in place."""
    xv, w, dst, res = _polsolve_args("pol_block_apply", x, "x", weights, out)
    _call("pxl_pol_block_apply_f64", xv, _ptr(w), _ptr(xv), _ptr(dst), xv.shape[1] * xv.shape[2])
    return res


# ---- the normal operator of the polarised map-maker; the iteration on top of it is mapmaker.py ----------------

def normal_pol(x: Enmap, w: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, out=None) -> Enmap:
    """y += P^T W P x in one pass (pxl_normal_car_pol_bilinear_f64): P the order-1 pointing matrix of sample_pol,
    W = diag(w) the (N,) sample weights, `x` a Float64 IQU CAR Enmap (3, ny, nx), skycoords and resp the (N, 2) batches of
    sample_pol.  out=None allocates zeros; a given `out` (Enmap or (3, ny, nx) tensor) is ACCUMULATED into and returned.  The
    call adds the same terms, bit for bit, as scatter_pol(w * sample_pol(x, skycoords, resp), skycoords, resp, out=out): only
    the order of the atomic adds into one pixel is unspecified, with scatter_bilinear's clause on the last bits.  A point
    whose position is not finite adds nothing; a non-finite pixel of x or weight makes the four taps of every point that
    reads it NaN in all three planes.  Full maps, order 1, Float64 and CAR only; `out` may not overlap x, w, skycoords or resp."""
    if not isinstance(x, Enmap):
        raise TypeError("normal_pol takes an Enmap")
    _car_only(x.wcs, "normal_pol")
    _iqu_map(x, "normal_pol")
    for t, noun in ((x.data, "maps"), (w, "w"), (skycoords, "skycoords")):
        _no_f32("normal_pol", t, noun)
    xv = _dev_f64(x.data, "map data")
    sky = _coords(skycoords, "skycoords", xv.device)
    r = _resp_arg("normal_pol", resp, sky)
    wv = _dev_f64(w, "w")
    if wv.dim() != 1 or wv.shape[0] != sky.shape[0] or wv.device != sky.device:
        raise ValueError("w must be (N,) on %s with N = %d" % (sky.device, sky.shape[0]))
    dst, res = _out_map(out, x.wcs, lambda: torch.zeros_like(xv), xv.device, shapes=(tuple(xv.shape),),
                        f32="normal_pol accumulates into Float64 maps", clear=(xv, wv, sky, r),
                        clear_msg="out overlaps x, w, skycoords or resp")
    _call("pxl_normal_car_pol_bilinear_f64", sky, _wcs_ref(x.wcs), _shape3((xv.shape[2], xv.shape[1]), 3), _ptr(xv), _ptr(dst),
          sky.shape[0], _ptr(sky), _ptr(r), _ptr(wv))
    return res


# ---- nearest-pixel (order 0) pointing and the one-pass binned IQU accumulation --------------------------------

def sample_nearest(m: Enmap, skycoords: torch.Tensor, src_rows=None, full_shape=None) -> torch.Tensor:
    """Nearest-pixel sample of every component of the Float64 CAR map `m` at a 2xN batch of (ra, dec)
    (pxl_sample_car_nearest_f64).  Returns (nc, N).  The position (x, y) is sample_bilinear's bit for bit; the pixel
    is i = floor(x) + (x - floor(x) >= 0.5), j likewise: pixel i owns [i - 0.5, i + 0.5), a tie goes to the higher index.
    Columns wrap on a full-circle map and are off the map outside [1, nx] otherwise; rows are on the map inside [1, ny].  The
    result is the pixel's value unchanged (no arithmetic: -0.0, subnormals, Inf and NaN come back as bits), +0.0 for a point
    that is not on the map, NaN where the position is not finite.  src_rows/full_shape as for sample_bilinear.  Float64 and
    CAR only."""
    return _sample_rows("sample_nearest", "pxl_sample_car_nearest_f64", m, skycoords, src_rows, full_shape, f32_first=True)


def scatter_nearest(vals: torch.Tensor, skycoords: torch.Tensor, shape, wcs, out=None, src_rows=None, full_shape=None) -> Enmap:
    """The transpose of sample_nearest (pxl_scatter_car_nearest_f64): add `vals` at a 2xN batch of (ra, dec) into
    a Float64 CAR map, each value to the one pixel sample_nearest reads, the value itself with no product -- binning, or a hit
    count map for vals = 1.  Arguments, `out` (ACCUMULATED into) and src_rows/full_shape as for scatter_bilinear.  A point
    that is not on the map, or whose position is not finite, adds nothing; a NaN value reaches exactly its one pixel per
    plane.  The adds are hardware FP64 atomics, with scatter_bilinear's clause on the last bits; pixels that receive
    nothing keep their bits.  Float64 and CAR only; `out` may not overlap vals or skycoords."""
    return _scatter_rows("scatter_nearest", "pxl_scatter_car_nearest_f64", vals, skycoords, shape, wcs, out, src_rows, full_shape)


def sample_pol_nearest(m: Enmap, skycoords: torch.Tensor, resp: torch.Tensor, src_rows=None, full_shape=None) -> torch.Tensor:
    """P m for the nearest-pixel polarised pointing matrix (pxl_sample_car_pol_nearest_f64): the (N,) samples
    out[k] = (s_I + q_k s_Q) + u_k s_U of the Float64 IQU CAR map `m`, with s = sample_nearest(m, skycoords, src_rows,
    full_shape) bit for bit, left to right without fma.  resp as for sample_pol.  Float64 and CAR only."""
    return _sample_rows("sample_pol_nearest", "pxl_sample_car_pol_nearest_f64", m, skycoords, src_rows, full_shape, pol=True, resp=resp,
                        f32_first=True)


def scatter_pol_nearest(vals: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, shape, wcs, out=None, src_rows=None,
                        full_shape=None) -> Enmap:
    """P^T d, the transpose of sample_pol_nearest (pxl_scatter_car_pol_nearest_f64): with v = vals[k] and
    (q, u) = resp[k], the one pixel of point k takes v in plane I, q v in plane Q and u v in plane U of a Float64 IQU CAR map
    (3, ny, nx), each exactly as scatter_nearest adds vals[c][k].  out (ACCUMULATED into), src_rows/full_shape as for
    scatter_nearest; the same atomics under the same clause.  `out` may not overlap vals, skycoords or resp."""
    return _scatter_pol("scatter_pol_nearest", 0, vals, skycoords, resp, shape, wcs, 0, out, False, src_rows, full_shape)


def scatter_pol_weights_nearest(w: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, shape, wcs, out=None, src_rows=None,
                                full_shape=None) -> Enmap:
    """The six planes II, IQ, IU, QQ, QU, UU of P^T W P for the nearest-pixel P, (6, ny, nx): scatter_pol_nearest's adds with
    w[k] times 1, q, u, q(q w), q(u w), u(u w).  With one pixel per point these blocks are ALL of P^T W P: pol_block_apply(x,
    weights) is P^T W P x.  Arguments as for scatter_pol_nearest."""
    return _scatter_pol("scatter_pol_weights_nearest", 1, w, skycoords, resp, shape, wcs, 0, out, False, src_rows, full_shape)


def bin_pol_nearest(d: torch.Tensor, w: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, shape, wcs, rhs=None, weights=None):
    """The map-making pass of nearest-pixel pointing, fused (pxl_bin_car_pol_nearest_f64): rhs += P^T (w d) and
    weights += the six planes of P^T W P, for the (N,) samples `d` with weights `w` at a 2xN batch of (ra, dec) with responses
    `resp`, in one pass of nine atomic adds per point.  Returns (rhs, weights): the (3, ny, nx) and (6, ny, nx) Float64 CAR
    Enmaps, zeros to start with when None, ACCUMULATED into and returned when given (Enmaps or tensors).  The call adds the
    same terms, bit for bit, as scatter_pol_nearest(w * d, ..., out=rhs) plus scatter_pol_weights_nearest(w, ..., out=weights):
    only the order of the atomic adds into one pixel is unspecified, with scatter_bilinear's clause on the last bits.  Full
    maps, Float64 and CAR only; rhs and weights may not overlap each other or d, w, skycoords, resp."""
    _car_only(wcs, "bin_pol_nearest")
    for t, noun in ((d, "d"), (w, "w"), (skycoords, "skycoords"), (resp, "resp")):
        _no_f32("bin_pol_nearest", t, noun)
    _sample_vectors("bin_pol_nearest", d, w)
    sky = _coords(skycoords, "skycoords", d.device, n=d.shape[0])
    r = _resp_arg("bin_pol_nearest", resp, sky)
    shp2, _row0, _nrows = _row_window(shape, None)
    ins = (d, w, sky, r)
    msg = "rhs and weights may not overlap each other or d, w, skycoords, resp"
    maps = []
    for given, planes in ((rhs, 3), (weights, 6)):
        oshape = (planes, shp2[1], shp2[0])
        maps.append(_out_map(given, wcs, lambda: torch.zeros(oshape, dtype=torch.float64, device=sky.device), sky.device,
                             shapes=(oshape,), f32="bin_pol_nearest accumulates into Float64 maps", clear=ins, clear_msg=msg))
    (rdst, rres), (wdst, wres) = maps
    if _overlap(rdst, wdst):
        raise ValueError(msg)
    _call("pxl_bin_car_pol_nearest_f64", sky, _wcs_ref(wcs), _shape3(shp2, 3), _ptr(rdst), _ptr(wdst), sky.shape[0], _ptr(sky), _ptr(r),
          _ptr(d), _ptr(w))
    return rres, wres


# ---- the two passes of the destriper; the map-maker on top of them is mapmaker.py ---------------------------------

def _baseline_args(what, w, skycoords, resp, shape, wcs, n_det, t0, baseline_len, n_base, d, a, mask):
    """The argument checks baseline_bin_pol_nearest and baseline_project_pol_nearest share.  Returns (sky, r, shp2, layout, ins):
    the coordinate and response batches, the map's (nx, ny), the integers (n_det, n_chunk, t0, baseline_len, n_base) and the
    tensors read (w, sky, resp, then whichever of d, a and the mask plane are given) that an output may not overlap."""
    _car_only(wcs, what)
    for t, noun in ((w, "w"), (skycoords, "skycoords"), (resp, "resp"), (d, "d"), (a, "a")):
        _no_f32(what, t, noun)
    if d is None and a is None:
        raise ValueError("%s needs d, a or both" % what)
    wv = _dev_f64(w, "w")
    if wv.dim() != 1:
        raise ValueError("w must be an (N,) tensor")
    sky = _coords(skycoords, "skycoords", wv.device, n=wv.shape[0])
    r = _resp_arg(what, resp, sky)
    n_det, t0, baseline_len, n_base = int(n_det), int(t0), int(baseline_len), int(n_base)
    if n_det < 1 or t0 < 0 or baseline_len < 1 or n_base < 0:
        raise ValueError("%s: n_det >= 1, t0 >= 0, baseline_len >= 1 and n_base >= 0 (got %d, %d, %d, %d)" % (what, n_det, t0, baseline_len, n_base))
    n = wv.shape[0]
    if n % n_det:
        raise ValueError("%s: the %d samples are not n_det = %d detectors of one chunk length" % (what, n, n_det))
    n_chunk = n // n_det
    if n_chunk and (t0 + n_chunk - 1) // baseline_len >= n_base:
        raise ValueError("%s: the chunk's times [%d, %d) reach past n_base = %d baselines of %d samples" % (what, t0, t0 + n_chunk, n_base, baseline_len))
    ins = [wv, sky, r]
    if d is not None:
        dv = _dev_f64(d, "d")
        if tuple(dv.shape) != (n,) or dv.device != wv.device:
            raise ValueError("d and w must be (N,) tensors on one device")
        ins.append(dv)
    if a is not None:
        av = _on(_dev_f64(a, "a"), "a", wv.device)
        if av.numel() != n_det * n_base:
            raise ValueError("%s: a holds n_det * n_base = %d amplitudes" % (what, n_det * n_base))
        ins.append(av)
    shp2, _row0, _nrows = _row_window(shape, None)
    if mask is not None:
        mv = mask.data if isinstance(mask, Enmap) else mask
        _no_f32(what, mv, "mask")
        mv = _on(_dev_f64(mv, "mask"), "mask", wv.device)
        if tuple(mv.shape) != (shp2[1], shp2[0]):
            raise ValueError("%s: mask is one (%d, %d) plane" % (what, shp2[1], shp2[0]))
        ins.append(mv)
    return sky, r, shp2, (n_det, n_chunk, t0, baseline_len, n_base), ins


def _opt_ptr(t):
    return None if t is None else _ptr(t.data if isinstance(t, Enmap) else t)


def baseline_bin_pol_nearest(w: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, shape, wcs, n_det, t0, baseline_len, n_base,
                             d=None, a=None, mask=None, out=None) -> Enmap:
    """The destriper's binning pass (pxl_baseline_bin_car_pol_nearest_f64): out += P^T (w o x) over the uncut samples
    of one time chunk, P the nearest-pixel polarised pointing matrix.  The chunk is detector-major as expand_pointing writes it:
    the (N,) weights `w`, (N, 2) skycoords and resp are times [t0, t0 + N / n_det) of n_det detectors, and sample k of detector
    det at chunk offset j lies in baseline b = det * n_base + (t0 + j) // baseline_len.  x = d (a None), a[b] (d None) or
    d - a[b] with one rounding; `a` holds n_det * n_base amplitudes.  A sample is cut where its position is not finite, where it
    is off the map, or where `mask` (an (ny, nx) Enmap or tensor, None: keep everything) is not > 0 at its pixel: it adds
    nothing, whatever its d.  Returns the (3, ny, nx) Float64 CAR Enmap, zeros to start with when out is None, ACCUMULATED into
    when given.  The call adds the same terms, bit for bit, as scatter_pol_nearest(w * x, ...) of the uncut samples, under
    the scatters' clause on the last bits.  Full maps, Float64 and CAR only; out may not overlap an input."""
    what = "baseline_bin_pol_nearest"
    sky, r, shp2, layout, ins = _baseline_args(what, w, skycoords, resp, shape, wcs, n_det, t0, baseline_len, n_base, d, a, mask)
    oshape = (3, shp2[1], shp2[0])
    dst, res = _out_map(out, wcs, lambda: torch.zeros(oshape, dtype=torch.float64, device=sky.device), sky.device, shapes=(oshape,),
                        f32="%s accumulates into Float64 maps" % what, clear=ins, clear_msg="out may not overlap w, skycoords, resp, d, a or mask")
    _call("pxl_baseline_bin_car_pol_nearest_f64", sky, _wcs_ref(wcs), _shape3(shp2, 3), _ptr(dst), _opt_ptr(mask), *layout, _ptr(sky), _ptr(r),
          _ptr(w), _opt_ptr(d), _opt_ptr(a))
    return res


def baseline_project_pol_nearest(w: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, shape, wcs, n_det, t0, baseline_len, n_base,
                                 d=None, a=None, m=None, mask=None, out=None) -> torch.Tensor:
    """The destriper's projection pass (pxl_baseline_project_car_pol_nearest_f64): out[b] += the sum over the uncut
    samples of baseline b in this chunk of w (x - P m), arguments, sample value x and cut rule as for baseline_bin_pol_nearest.
    `m` is a (3, ny, nx) Float64 IQU Enmap or tensor and P m is sample_pol_nearest's value, operation for operation; m=None
    skips the subtraction (the term is w x).  Returns the (n_det * n_base,) Float64 tensor: zeros to start with when out is None,
    ACCUMULATED into when given, so a baseline that spans chunks is summed chunk by chunk.  No atomics: every (baseline, chunk)
    segment is summed by one owner in a fixed order, the same arguments give the same bits, and a baseline whose samples here
    are all cut keeps its bits.  Full maps, Float64 and CAR only; out may not overlap an input."""
    what = "baseline_project_pol_nearest"
    sky, r, shp2, layout, ins = _baseline_args(what, w, skycoords, resp, shape, wcs, n_det, t0, baseline_len, n_base, d, a, mask)
    if m is not None:
        mv = m.data if isinstance(m, Enmap) else m
        _no_f32(what, mv, "maps")
        mv = _on(_dev_f64(mv, "m"), "m", sky.device)
        if tuple(mv.shape) != (3, shp2[1], shp2[0]):
            raise ValueError("%s: m is a (3, %d, %d) IQU map" % (what, shp2[1], shp2[0]))
        ins.append(mv)
    nb = layout[0] * layout[4]
    if out is None:
        out = torch.zeros((nb,), dtype=torch.float64, device=sky.device)
    _no_f32(what, out, "out")
    dst = _on(_dev_f64(out, "out"), "out", sky.device)
    if tuple(dst.shape) != (nb,):
        raise ValueError("%s: out holds n_det * n_base = %d amplitudes, as an (%d,) tensor" % (what, nb, nb))
    if any(_overlap(dst, t) for t in ins):
        raise ValueError("out may not overlap w, skycoords, resp, d, a, m or mask")
    _call("pxl_baseline_project_car_pol_nearest_f64", sky, _wcs_ref(wcs), _shape3(shp2, 3), _opt_ptr(m), _opt_ptr(mask), *layout, _ptr(sky),
          _ptr(r), _ptr(w), _opt_ptr(d), _opt_ptr(a), _ptr(dst))
    return dst


# ---- the per-scan polynomial filter; the filter-and-bin map-maker on top of it is mapmaker.py ----------------------

def _seg_start(what, seg_start, nt, name="seg_start", axis="T"):
    """The host list of segment offsets: a sequence of integers or a CPU integer tensor, at least one, non-decreasing, in [0, nt].
    name, axis: the same checks for modefilter_tod's grp_start on the detector axis."""
    if isinstance(seg_start, torch.Tensor):
        if seg_start.is_cuda or seg_start.is_floating_point() or seg_start.dim() != 1:
            raise ValueError("%s: %s is a host sequence of integers or a 1-D CPU integer tensor" % (what, name))
    seg_start = seg_start.tolist() if hasattr(seg_start, "tolist") else list(seg_start)
    segs = [int(v) for v in seg_start]
    if any(a != b for a, b in zip(segs, seg_start)):
        raise ValueError("%s: %s holds integers" % (what, name))
    if not segs:
        raise ValueError("%s: %s holds n_%s + 1 offsets, at least one" % (what, name, name[:3]))
    if any(b < a for a, b in zip(segs, segs[1:])):
        raise ValueError("%s: %s must be non-decreasing" % (what, name))
    if segs[0] < 0 or segs[-1] > nt:
        raise ValueError("%s: %s must lie inside [0, %s] = [0, %d]" % (what, name, axis, nt))
    return segs


def _tod_shape(what, tod):
    """(D, T) of the Float64 timestream a filter takes.  A host check, as everything is that a filter does before _tod_filter_args."""
    _no_f32(what, tod, "tod")
    if not isinstance(tod, torch.Tensor) or tod.dim() != 2:
        raise ValueError("%s: tod is a (D, T) tensor" % what)
    return tod.shape


def _tod_filter_args(what, tod, w, out, rcond_min, also=()):
    """What the timestream filters share once their own host checks are through: rcond_min, the last check that needs no device, then
    the (D, T) `tod` on the GPU, the weights spread from (D,) if need be, and `out`, which may be tod itself and may overlap neither
    tod otherwise, nor w, nor any of `also`: (name, tensor) pairs of further device inputs (modefilter's modes), checked as tod is.
    Returns (d, wv, dst, rmin)."""
    rmin = float(rcond_min)
    if not (0.0 <= rmin < 1.0):
        raise ValueError("rcond_min must lie in [0, 1), not %r" % (rcond_min,))
    nd, nt = tod.shape
    d = _dev_f64(tod, "tod")
    for name, t in also:
        _on(_dev_f64(t, name), name, d.device)
    wv = None
    if w is not None:
        wv = _on(_f64(w, "w", what), "w", d.device)
        if tuple(wv.shape) == (nd,):
            wv = wv[:, None].expand(nd, nt).contiguous()
        elif tuple(wv.shape) != (nd, nt):
            raise ValueError("%s: w is (D, T) or (D,) for this tod" % what)
    if out is None:
        out = torch.empty_like(d)
    dst = _on(_f64(out, "out", what), "out", d.device)
    if tuple(dst.shape) != (nd, nt):
        raise ValueError("%s: out is a (%d, %d) tensor" % (what, nd, nt))
    if (dst.data_ptr() != d.data_ptr() and _overlap(dst, d)) or (wv is not None and _overlap(dst, wv)) or any(_overlap(dst, t) for _n, t in also):
        raise ValueError("out may be tod itself (in place) and may not overlap tod otherwise, nor w" + "".join(", nor " + n for n, _t in also))
    return d, wv, dst, rmin


def _fit_info(wanted, device, shape, count_shape):
    """The two optional outputs of a filter's fit, zeroed: the Float64 coefficients and the int64 count of those fitted; (None, None)
    where they are not asked for."""
    if not wanted:
        return None, None
    return torch.zeros(shape, dtype=torch.float64, device=device), torch.zeros(count_shape, dtype=torch.int64, device=device)


def polyfilter_tod(tod: torch.Tensor, seg_start, order, w=None, out=None, rcond_min=1e-10, return_fit_info=False):
    """The per-scan polynomial filter (pxl_tod_polyfilter_f64): for every detector of the (D, T) Float64 timestream
    `tod` and every segment [seg_start[s], seg_start[s+1]) -- a scan, from one turnaround to the next -- a Legendre polynomial of
    degree <= `order` (0 to 7) is fitted by weighted least squares to the samples with w > 0 and subtracted from ALL samples of
    the segment: "fit here, subtract everywhere".  seg_start: n_seg + 1 offsets shared by all detectors, a host sequence of
    integers or a CPU integer tensor, non-decreasing and inside [0, T] (ValueError otherwise), uploaded by this call; samples
    before the first and from the last offset on are copied.  w: the fit weights, (D, T), one per detector (D,), or None for
    1.0 everywhere; a sample whose weight is not > 0 (zero, negative, NaN) takes no part in the fit and its value is never read
    into it, so a NaN under a zero weight stays in its own sample.  out: the (D, T) tensor to write (None: a new one); out=tod
    filters in place; any other overlap is refused.

    The fit is truncated where the normal equations lose rank: pivot i of their LDL^T, taken in the Legendre order, is accepted
    when D_i > rcond_min * G_ii, and the first rejected pivot ends the fit, so a segment with n live samples is fitted with at
    most n coefficients and an all-cut segment is copied.  A pivot ratio r costs about log10(1 / r) of the coefficients' 16
    digits, so the default rcond_min = 1e-10 leaves at least five.  With return_fit_info the call returns (out, coeffs,
    n_used): the (D, n_seg, order + 1) Legendre coefficients on x_j = ((2j + 1) - L) / L of each segment of L samples, +0.0
    from n_used on, and the (D, n_seg) int64 count of coefficients fitted.  No atomics: the same arguments give the same bits
    (the header states every operation).  Float64, one device."""
    what = "polyfilter_tod"
    nd, nt = _tod_shape(what, tod)
    order = int(order)
    if not 0 <= order <= 7:
        raise ValueError("%s: order must be 0 to 7, not %d" % (what, order))
    segs = _seg_start(what, seg_start, nt)
    nseg = len(segs) - 1
    d, wv, dst, rmin = _tod_filter_args(what, tod, w, out, rcond_min)
    coeffs, n_used = _fit_info(return_fit_info, d.device, (nd, nseg, order + 1), (nd, nseg))
    seg_dev = torch.tensor(segs, dtype=torch.int64).to(d.device)
    _call("pxl_tod_polyfilter_f64", d, nd, nt, nseg, _ptr(seg_dev), order, rmin, _ptr(d), _opt_ptr(wv), _ptr(dst), _opt_ptr(coeffs), _opt_ptr(n_used))
    return (dst, coeffs, n_used) if return_fit_info else dst


# ---- the detector-mode filter: the same projection across detectors, per time sample and detector group ------------

def modefilter_tod(tod: torch.Tensor, modes, w=None, grp_start=None, out=None, rcond_min=1e-10, return_fit_info=False):
    """The detector-mode filter (pxl_tod_modefilter_f64): for every time sample of the (D, T) Float64 timestream `tod`
    and every detector group [grp_start[g], grp_start[g+1]), K amplitudes c are fitted by weighted least squares to the group's
    detectors with w > 0 on the couplings `modes` -- F, a (D, K) tensor, or (D,) for K = 1; K is 1 to 8 -- and F c is subtracted
    from ALL detectors of the group: "fit on the live detectors, subtract everywhere".  F = 1 or the gains is the common mode,
    F = (1, x_d, y_d) a plane across the focal plane, F = eigenvectors of the caller's a PCA filter.  grp_start: n_grp + 1
    detector offsets, a host sequence of integers or a CPU integer tensor, non-decreasing and inside [0, D] (ValueError
    otherwise), uploaded by this call; None is one group of all detectors; detectors before the first and from the last offset
    on are copied.  w: the fit weights, (D, T), one per detector (D,), or None for 1.0 everywhere; a sample whose weight is not
    > 0 (zero, negative, NaN) takes no part in the fit and its value is never read into it, so a NaN under a zero weight stays
    in its own sample.  out: the (D, T) tensor to write (None: a new one); out=tod filters in place; any other overlap is refused.

    The fit is truncated where the normal equations lose rank, by polyfilter_tod's rule in the caller's mode order: pivot i of
    their LDL^T is accepted when D_i > rcond_min * G_ii and the first rejected pivot ends the fit, so a column with n live
    detectors is fitted with at most n modes and an all-cut column is copied.  With return_fit_info the call returns (out, amps,
    n_used): the (n_grp, K, T) amplitudes, +0.0 from n_used on, and the (n_grp, T) int64 count of modes fitted.  No atomics: the
    same arguments give the same bits (the header states every operation).  Float64, one device."""
    return _modefilter("modefilter_tod", tod, modes, w, grp_start, out, rcond_min, return_fit_info)


def _modefilter(what, tod, modes, w, grp_start, out, rcond_min, return_fit_info):
    """modefilter_tod in the name of `what`."""
    nd, nt = _tod_shape(what, tod)
    if not isinstance(modes, torch.Tensor) or modes.dim() not in (1, 2) or modes.shape[0] != nd:
        raise ValueError("%s: modes is a (D, K) tensor, or (D,) for one mode" % what)
    _no_f32(what, modes, "modes")
    nk = 1 if modes.dim() == 1 else int(modes.shape[1])
    if not 1 <= nk <= 8:
        raise ValueError("%s: modes holds 1 to 8 modes, not %d" % (what, nk))
    grps = [0, nd] if grp_start is None else _seg_start(what, grp_start, nd, "grp_start", "D")
    ngrp = len(grps) - 1
    d, wv, dst, rmin = _tod_filter_args(what, tod, w, out, rcond_min, also=(("modes", modes),))
    amps, n_used = _fit_info(return_fit_info, d.device, (ngrp, nk, nt), (ngrp, nt))
    grp_dev = torch.tensor(grps, dtype=torch.int64).to(d.device)
    _call("pxl_tod_modefilter_f64", d, nd, nt, ngrp, _ptr(grp_dev), nk, _ptr(modes), rmin, _ptr(d), _opt_ptr(wv), _ptr(dst), _opt_ptr(amps),
          _opt_ptr(n_used))
    return (dst, amps, n_used) if return_fit_info else dst


def common_mode_tod(tod: torch.Tensor, w=None, gains=None, grp_start=None, out=None, rcond_min=1e-10, return_fit_info=False):
    """Common-mode removal: modefilter_tod with the one mode `gains`, a (D,) tensor, or ones where it is None -- per time sample and
    detector group the weighted mean of the live detectors (in units of their gains) is subtracted from every detector of the
    group.  The other arguments and the result are modefilter_tod's."""
    what = "common_mode_tod"
    if not isinstance(tod, torch.Tensor) or tod.dim() != 2:
        raise ValueError("%s: tod is a (D, T) tensor" % what)
    if gains is None:
        gains = torch.ones((tod.shape[0],), dtype=torch.float64, device=tod.device)
    elif not isinstance(gains, torch.Tensor) or gains.dim() != 1:
        raise ValueError("%s: gains is a (D,) tensor" % what)
    return _modefilter(what, tod, gains, w, grp_start, out, rcond_min, return_fit_info)


# ---- the binned-template filter: the same projection on the samples that share a bin of scan phase --------------------

def _bin_index(what, index):
    """The (T,) integer tensor of a bin index, from a tensor or an array, on the device it already lives on."""
    if not isinstance(index, torch.Tensor):
        index = torch.as_tensor(index)
    if index.dim() != 1 or index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
        raise ValueError("%s: index is a (T,) tensor or array of integers" % what)
    return index.to(torch.int64)


class _BinPlan(tuple):
    """The (order, bin_start) pair as bin_plan returns it.  binfilter_tod notes on it the check it made (`checked`: for which T and
    which versions of the two tensors, and the host offsets it read), so that a plan used for many calls is checked once."""
    checked = None


def bin_plan(index, n_bin, device=None):
    """The plan that binfilter_tod takes, from one bin index per time sample: (order, bin_start), two int64 tensors.  index: a (T,)
    integer tensor or array; a value outside [0, n_bin) means "filter nothing here" (turnarounds).  With key = index where it is
    in range and n_bin elsewhere, order is the STABLE argsort of key -- time order inside every bin, the unfiltered samples last
    -- and bin_start[b], b = 0 .. n_bin, is the number of samples with key < b, so bin b is order[bin_start[b]:bin_start[b+1]].
    Built with torch on `device` (None: where index lives; binfilter_tod uploads a host plan).  ValueError for n_bin < 1 and for
    an index that is not of integers."""
    what = "bin_plan"
    n_bin = int(n_bin)
    if n_bin < 1:
        raise ValueError("%s: n_bin must be at least 1, not %d" % (what, n_bin))
    key = _bin_index(what, index)
    if device is not None:
        key = key.to(device)
    key = torch.where((key >= 0) & (key < n_bin), key, torch.full_like(key, n_bin))
    order = torch.sort(key, stable=True).indices
    counts = torch.bincount(key, minlength=n_bin + 1)[:n_bin]
    bin_start = torch.cat([torch.zeros(1, dtype=torch.int64, device=key.device), torch.cumsum(counts, 0)])
    return _BinPlan((order, bin_start))


def scan_bins(az, n_bin, lo, hi, split_direction=False):
    """The usual bin index of a scan: one int64 per sample of the (T,) Float64 azimuth `az` (a tensor on any device, or an array),
    for bin_plan.  In Float64, k = floor((az - lo) * (n_bin / (hi - lo))), lowered to n_bin - 1 where the product rounds up to
    n_bin below hi; -1 where az is outside [lo, hi) or not finite.  With split_direction a sample t whose central difference
    az[min(t + 1, T - 1)] - az[max(t - 1, 0)] is negative (a NaN is not) gets n_bin added, so that the two sweep directions have
    their own templates: the caller then passes 2 * n_bin bins to bin_plan.  ValueError unless n_bin >= 1 and lo < hi, finite."""
    what = "scan_bins"
    n_bin, lo, hi = int(n_bin), float(lo), float(hi)
    if n_bin < 1:
        raise ValueError("%s: n_bin must be at least 1, not %d" % (what, n_bin))
    if not (lo < hi and hi - lo < float("inf")):
        raise ValueError("%s: lo < hi, both finite" % what)
    az = torch.as_tensor(az)
    if az.dim() != 1 or az.dtype != torch.float64:
        raise ValueError("%s: az is a (T,) Float64 tensor or array" % what)
    inside = (az >= lo) & (az < hi)
    k = torch.floor((az - lo) * (n_bin / (hi - lo)))
    k = torch.where(inside, k, torch.zeros_like(k)).to(torch.int64).clamp_(max=n_bin - 1)
    if split_direction and az.numel():
        t = torch.arange(az.numel(), device=az.device)
        back = (az[(t + 1).clamp_(max=az.numel() - 1)] - az[(t - 1).clamp_(min=0)]) < 0
        k = k + n_bin * back.to(torch.int64)
    return torch.where(inside, k, torch.full_like(k, -1))


def _bin_plan_arg(what, plan, n_bin, nt):
    """binfilter_tod's plan on the host side: (order, offsets) -- the int64 tensor of T sample indices, wherever it lives, and the
    host list of n_bin + 1 offsets.  plan is a (T,) index with n_bin given, built here by bin_plan, or the pair bin_plan
    returns, checked: T entries, non-decreasing offsets inside [0, T], and order a permutation (one sort and one compare).  The
    check reads the device, so a pair that bin_plan made remembers it until one of its tensors is written to."""
    if n_bin is not None:
        index = _bin_index(what, plan)
        if index.numel() != nt:
            raise ValueError("%s: the bin index holds one entry per time sample, T = %d" % (what, nt))
        order, bin_start = bin_plan(index, n_bin)
        return order, bin_start.tolist()
    if not (isinstance(plan, (tuple, list)) and len(plan) == 2 and all(isinstance(p, torch.Tensor) for p in plan)):
        raise ValueError("%s: plan is the (order, bin_start) pair of bin_plan, or a (T,) bin index with n_bin given" % what)
    order, bin_start = plan
    stamp = (nt, order.data_ptr(), order._version, bin_start.data_ptr(), bin_start._version)
    if isinstance(plan, _BinPlan) and plan.checked is not None and plan.checked[0] == stamp:
        return order, plan.checked[1]
    if order.dim() != 1 or order.dtype != torch.int64 or bin_start.dim() != 1 or bin_start.dtype != torch.int64:
        raise ValueError("%s: order and bin_start are 1-D int64 tensors" % what)
    if order.numel() != nt:
        raise ValueError("%s: order holds one entry per time sample, T = %d, not %d" % (what, nt, order.numel()))
    segs = _seg_start(what, bin_start.tolist(), nt, "bin_start")
    if not torch.equal(torch.sort(order).values, torch.arange(nt, dtype=torch.int64, device=order.device)):
        raise ValueError("%s: order must be a permutation of the T = %d time samples" % (what, nt))
    if isinstance(plan, _BinPlan):
        plan.checked = (stamp, segs)
    return order, segs


def binfilter_tod(tod: torch.Tensor, plan, n_bin=None, w=None, out=None, return_fit_info=False):
    """The binned-template filter (pxl_tod_binfilter_f64): for every detector of the (D, T) Float64 timestream `tod`
    and every bin of `plan` the weighted mean of the bin's samples with w > 0 is subtracted from ALL samples of the bin: "fit
    here, subtract everywhere" with one constant per (detector, bin).  It removes what is a function of the bin alone -- ground
    pickup binned in azimuth (scan_bins), a half-wave plate's synchronous signal binned in its angle, the difference between the
    two sweep directions -- which neither a polynomial in time nor a mode across detectors can.  plan: the (order, bin_start)
    pair of bin_plan, shared by all detectors and checked here on the host (T entries, non-decreasing offsets inside [0, T],
    order a permutation; ValueError otherwise), or a (T,) integer bin index with n_bin given, from which bin_plan builds the pair
    here; a sample in no bin is copied.  w: the fit weights, (D, T), one per detector (D,), or None for 1.0 everywhere; a sample
    whose weight is not > 0 (zero, negative, NaN) takes no part in the mean and its value is never read into it, so a NaN under
    a zero weight stays in its own sample.  out: the (D, T) tensor to write (None: a new one); out=tod filters in place; any
    other overlap is refused.

    A bin whose live weights do not sum to a positive, finite number is copied.  With return_fit_info the call returns (out,
    means, n_used): the (D, n_bin) means, +0.0 where none was fitted, and the (D, n_bin) int64 count, 1 or 0.  No atomics: the
    same arguments give the same bits (the header states every operation).  Float64, one device."""
    what = "binfilter_tod"
    nd, nt = _tod_shape(what, tod)
    order, segs = _bin_plan_arg(what, plan, n_bin, nt)
    nbin = len(segs) - 1
    d, wv, dst, _rmin = _tod_filter_args(what, tod, w, out, 0.0)
    means, n_used = _fit_info(return_fit_info, d.device, (nd, nbin), (nd, nbin))
    order_dev = order.to(d.device).contiguous()
    if n_bin is None and plan[1].device == d.device and plan[1].is_contiguous():
        bin_dev = plan[1]                                   # the checked offsets, where they already are
    else:
        bin_dev = torch.tensor(segs, dtype=torch.int64).to(d.device)
    _call("pxl_tod_binfilter_f64", d, nd, nt, nbin, _ptr(bin_dev), _ptr(order_dev), _ptr(d), _opt_ptr(wv), _ptr(dst), _opt_ptr(means), _opt_ptr(n_used))
    return (dst, means, n_used) if return_fit_info else dst


# ---- the banded-Toeplitz noise weight: N^-1 x of stationary correlated noise, what the ML map-maker is built on -----

TOEPLITZ_LAMBDA_MAX = 4096


def toeplitz_tod(tod: torch.Tensor, kernel: torch.Tensor, seg_start=None, w=None, out=None):
    """The banded-Toeplitz noise weight (pxl_tod_toeplitz_f64): out = G T G tod, the time-domain inverse covariance
    N^-1 of a stationary correlated noise process applied to the (D, T) Float64 timestream `tod`.  T is one symmetric banded
    Toeplitz block per detector and segment [seg_start[s], seg_start[s+1]) -- a scan; the blocks do not couple scans -- with the
    off-diagonals `kernel`: (D, lambda + 1) Float64 on the device of tod, or (lambda + 1,) for every detector; kernel[r][k] = c_k,
    lambda = 0 to 4096 (noise_kernel_from_psd makes one from a noise spectrum).  G zeroes the cut samples, on both sides ("gappy
    Toeplitz"): a sample is LIVE where it lies in a segment and w > 0 (zero, negative and NaN are not); w is (D, T), one per
    detector (D,), or None for every sample.  seg_start: n_seg + 1 offsets shared by all detectors, as for polyfilter_tod (a
    host sequence of integers or a CPU integer tensor, non-decreasing, inside [0, T]; ValueError otherwise); None is the one
    segment [0, T].

    For a live sample t, with z = tod at the live samples of t's segment and +0.0 everywhere else,
    out_t = c_0 z_t + sum_(k = 1 .. lambda) c_k (z_(t-k) + z_(t+k)), summed in that order, every operation rounded once.  A sample
    that is not live gets +0.0 exactly: this is a weight, so a cut sample weighs nothing (the filters copy theirs).  The value of
    tod under a cut is never read into a sum, so a NaN there stays out; a non-finite LIVE sample reaches the live samples within
    lambda of it in its segment and no others.  out: the (D, T) tensor to write (None: a new one); it may not overlap tod at all
    -- an output reads its neighbours, so there is no in-place form -- nor kernel or w.  No atomics: the bits are fixed by the
    arguments.  Float64, one device."""
    what = "toeplitz_tod"
    nd, nt = _tod_shape(what, tod)
    _no_f32(what, kernel, "kernel")
    if not isinstance(kernel, torch.Tensor) or kernel.dim() not in (1, 2) or kernel.shape[-1] < 1 or (kernel.dim() == 2 and kernel.shape[0] != nd):
        raise ValueError("%s: kernel is a (D, lambda + 1) tensor, or (lambda + 1,) for every detector" % what)
    lam = int(kernel.shape[-1]) - 1
    if lam > TOEPLITZ_LAMBDA_MAX:
        raise ValueError("%s: lambda must be 0 to %d, not %d" % (what, TOEPLITZ_LAMBDA_MAX, lam))
    segs = [0, nt] if seg_start is None else _seg_start(what, seg_start, nt)
    if out is tod:
        raise ValueError("%s: out may not be tod (an output reads its neighbours: there is no in-place form)" % what)
    d = _dev_f64(tod, "tod")
    kv = _on(_dev_f64(kernel, "kernel"), "kernel", d.device)
    if kv.dim() == 1:
        kv = kv[None, :].expand(nd, lam + 1).contiguous()
    wv = None
    if w is not None:
        wv = _on(_f64(w, "w", what), "w", d.device)
        if tuple(wv.shape) == (nd,):
            wv = wv[:, None].expand(nd, nt).contiguous()
        elif tuple(wv.shape) != (nd, nt):
            raise ValueError("%s: w is (D, T) or (D,) for this tod" % what)
    if out is None:
        out = torch.empty_like(d)
    dst = _on(_f64(out, "out", what), "out", d.device)
    if tuple(dst.shape) != (nd, nt):
        raise ValueError("%s: out is a (%d, %d) tensor" % (what, nd, nt))
    if _overlap(dst, d) or _overlap(dst, kv) or (wv is not None and _overlap(dst, wv)):
        raise ValueError("%s: out may not overlap tod, kernel or w" % what)
    seg_dev = torch.tensor(segs, dtype=torch.int64).to(d.device)
    _call("pxl_tod_toeplitz_f64", d, nd, nt, len(segs) - 1, _ptr(seg_dev), lam, _ptr(kv), _ptr(d), _opt_ptr(wv), _ptr(dst))
    return dst


def noise_kernel_from_psd(psd, lam, n_fft=None) -> torch.Tensor:
    """The kernel of toeplitz_tod from a noise power spectrum, on the host (numpy; no device, no library call).  psd: (D, n_fft // 2 + 1)
    or one row (n_fft // 2 + 1,), a tensor or an array: the one-sided noise power per sample at the frequencies rfftfreq(n_fft),
    every value finite and > 0 (ValueError otherwise); n_fft=None is the even length 2 (psd.shape[-1] - 1).  lam: lambda, 0 to
    min(4096, n_fft // 2).  Returns the Float64 CPU tensor (D, lam + 1), or (lam + 1,) for one row,

        c_k = irfft(1 / psd, n_fft)[k] * (1 - k / (lam + 1)),      k = 0 .. lam:

    the autocorrelation of the inverse spectrum -- for white noise of variance sigma^2, c_0 = 1 / sigma^2 and nothing else -- cut
    off at lam under a Bartlett (triangular) taper.

    WHY BARTLETT.  Conjugate gradients needs N^-1 = G T G positive semi-definite.  A symmetric Toeplitz matrix of any size is
    positive semi-definite if the spectrum of its kernel, sum_k c_|k| e^(i k f), is non-negative at every f.  The spectrum of the
    tapered kernel is the convolution of the spectrum of irfft(1 / psd) -- the values 1 / psd > 0 at the n_fft frequencies f_m --
    with the transform W of the taper: (1 / n_fft) sum_m W(f - f_m) / psd_m.  The Bartlett window's transform is the Fejer
    kernel, sin^2((lam + 1) f / 2) / ((lam + 1) sin^2(f / 2)) >= 0.  A convolution of two non-negative functions is non-negative,
    so every finite section of T is positive semi-definite, and with it every G T G, for any cuts and any segments.  The plain
    truncation at lam is the convolution with the Dirichlet kernel, which changes sign: for a steep 1 / f spectrum the
    truncated kernel's spectrum goes negative near f = 0 and T is indefinite (tests/test_toeplitz_ref.py holds a case).  The
    price is resolution: the taper smooths 1 / psd over about 2 pi / (lam + 1), so lam must reach past the knee's correlation
    length for the weight to tell the drift from the sky."""
    import numpy as np
    a = psd.detach().cpu().numpy() if isinstance(psd, torch.Tensor) else np.asarray(psd)
    if a.ndim not in (1, 2) or a.shape[-1] < 1 or not np.issubdtype(a.dtype, np.floating):
        raise ValueError("noise_kernel_from_psd: psd is a (D, n_fft // 2 + 1) array of floats, or one row")
    a = a.astype(np.float64)
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError("noise_kernel_from_psd: every value of psd must be finite and > 0")
    nf = a.shape[-1]
    n_fft = 2 * (nf - 1) if n_fft is None else int(n_fft)
    if n_fft < 1 or n_fft // 2 + 1 != nf:
        raise ValueError("noise_kernel_from_psd: psd holds n_fft // 2 + 1 = %d values for n_fft = %d, not %d" % (n_fft // 2 + 1, n_fft, nf))
    lam = int(lam)
    if not 0 <= lam <= min(TOEPLITZ_LAMBDA_MAX, n_fft // 2):
        raise ValueError("noise_kernel_from_psd: lam must be 0 to min(%d, n_fft // 2 = %d), not %d" % (TOEPLITZ_LAMBDA_MAX, n_fft // 2, lam))
    k = np.arange(lam + 1, dtype=np.float64)
    c = np.fft.irfft(1.0 / a, n=n_fft, axis=-1)[..., :lam + 1] * (1.0 - k / (lam + 1))
    return torch.from_numpy(np.ascontiguousarray(c))


# ---- the gappy autocovariance: the noise estimate that makes the Toeplitz weight's kernel from the data itself ---------

def _lam(what, lam):
    if isinstance(lam, bool) or not isinstance(lam, int) or not 0 <= lam <= TOEPLITZ_LAMBDA_MAX:
        raise ValueError("%s: lam must be an integer 0 to %d, not %r" % (what, TOEPLITZ_LAMBDA_MAX, lam))
    return lam


def autocov_tod(tod: torch.Tensor, lam, seg_start=None, w=None, return_pairs=True):
    """The gappy autocovariance of the (D, T) Float64 timestream `tod` up to lag `lam`, 0 to 4096 (pxl_tod_autocov_f64, DESIGN
    4.22).  Segments, cuts and their arguments are toeplitz_tod's: seg_start the n_seg + 1 offsets of the scans (None: the one
    segment [0, T]), w (D, T), one per detector (D,), or None; a sample is LIVE where it lies in a segment and w > 0 (zero,
    negative and NaN are not).  Returns (sums, pairs), or sums alone with return_pairs=False: the (D, lam + 1) Float64

        sums[r][k] = sum of tod[r][t] * tod[r][t + k] over the t with t and t + k live in the SAME scan

    and the (D, lam + 1) int64 number of those pairs, exact; +0.0 and 0 where there is none.  The scans are not coupled, and the
    value of tod under a cut is never read into a sum, so a NaN there stays out; a non-finite LIVE sample makes lag 0 of its own
    detector non-finite, possibly its other lags, and touches no other detector.  The order of every sum follows lam, T and
    seg_start alone (the header states it), so a detector has the same bits alone as in any batch, and two calls give the same
    bits: no atomics.  noise_psd_from_autocov makes the spectrum of it.  Float64, one device."""
    what = "autocov_tod"
    nd, nt = _tod_shape(what, tod)
    lam = _lam(what, lam)
    segs = [0, nt] if seg_start is None else _seg_start(what, seg_start, nt)
    d = _dev_f64(tod, "tod")
    wv = None
    if w is not None:
        wv = _on(_f64(w, "w", what), "w", d.device)
        if tuple(wv.shape) == (nd,):
            wv = wv[:, None].expand(nd, nt).contiguous()
        elif tuple(wv.shape) != (nd, nt):
            raise ValueError("%s: w is (D, T) or (D,) for this tod" % what)
        wv = wv.contiguous()
    sums = torch.empty((nd, lam + 1), dtype=torch.float64, device=d.device)
    pairs = torch.empty((nd, lam + 1), dtype=torch.int64, device=d.device) if return_pairs else None
    seg_dev = torch.tensor(segs, dtype=torch.int64).to(d.device)
    _call("pxl_tod_autocov_f64", d, nd, nt, len(segs) - 1, _ptr(seg_dev), lam, _ptr(d), _opt_ptr(wv), _ptr(sums), _opt_ptr(pairs))
    return (sums, pairs) if return_pairs else sums


def noise_psd_from_autocov(sums, pairs, n_fft=None, normalise="biased", floor=1e-3):
    """The noise power spectrum of autocov_tod's (sums, pairs), on the host (numpy; no device, no library call), ready for
    noise_kernel_from_psd.  sums: (D, lam + 1) floats, or one row; pairs: the same shape, integers; tensors or arrays.  Returns
    (psd, n_floored): the Float64 array (D, n_fft // 2 + 1) (one row for one row), every value finite and > 0, and per row the
    number of values that had to be raised.

        r_k = sums_k / pairs_0          normalise="biased"  (the default)
        r_k = sums_k / pairs_k          normalise="pairs", +0.0 where pairs_k = 0
        psd_m = r_0 + 2 sum_(k = 1 .. lam) (1 - k / (lam + 1)) r_k cos(2 pi m k / n_fft),      m = 0 .. n_fft // 2,

    one rfft of the symmetric sequence.  n_fft=None is the smallest power of two >= 2 (lam + 1); an n_fft <= 2 lam cannot hold
    the sequence and is refused.  Values below floor * (the row's median) are raised to it and counted.  A detector with
    pairs_0 = 0 (no live sample), a non-finite sum, or a spectrum whose median is not positive (only "pairs" can have one)
    raises ValueError naming it.

    WHY "biased".  sums_k of the zero-filled live samples z is the autocorrelation of a finite sequence, one per scan, so its
    transform is sum over the scans of |Z(f)|^2 >= 0, whatever the cuts.  Dividing every lag by the same pairs_0 keeps that, and
    the Bartlett taper multiplies it by a sequence whose own transform, the Fejer kernel, is >= 0 (noise_kernel_from_psd's
    argument): the spectrum is non-negative by construction, to rounding, and the kernel made of it positive semi-definite, which
    conjugate gradients needs.  "pairs" is unbiased lag by lag, but a sequence of ratios with different denominators is no
    autocorrelation of anything.  On the ML map's test case (1/f noise, scans of 1000 samples, five seeds) both work at lam =
    64 (map rms error 0.389 / 0.546 / 0.328 / 0.540 / 0.365 biased, 0.420 / 0.547 / 0.325 / 0.556 / 0.370 pairs); at lam = 256
    the "pairs" spectrum goes negative (minimum -0.19, 15 values floored) and its map, 0.735, is WORSE than the binned one, 0.590,
    while the biased form stays positive and gives 0.396 / 0.548 / 0.321 / 0.547 / 0.358."""
    import numpy as np
    what = "noise_psd_from_autocov"
    s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    n = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if s.ndim not in (1, 2) or s.shape[-1] < 1 or not np.issubdtype(s.dtype, np.floating):
        raise ValueError("%s: sums is a (D, lam + 1) array of floats, or one row" % what)
    if n.shape != s.shape or not np.issubdtype(n.dtype, np.integer):
        raise ValueError("%s: pairs is an array of integers of the shape of sums, %r" % (what, s.shape))
    if normalise not in ("biased", "pairs"):
        raise ValueError("%s: normalise is \"biased\" or \"pairs\", not %r" % (what, normalise))
    if not (isinstance(floor, (int, float)) and 0 < floor < 1):
        raise ValueError("%s: floor must lie in (0, 1), not %r" % (what, floor))
    lam = s.shape[-1] - 1
    if n_fft is None:
        n_fft = 2
        while n_fft < 2 * (lam + 1):
            n_fft *= 2
    n_fft = int(n_fft)
    if n_fft <= 2 * lam:
        raise ValueError("%s: n_fft must exceed 2 lam = %d to hold the symmetric sequence, not %d" % (what, 2 * lam, n_fft))
    s2, n2 = np.atleast_2d(s.astype(np.float64)), np.atleast_2d(n)
    for det in range(s2.shape[0]):
        if n2[det, 0] <= 0:
            raise ValueError("%s: detector %d has no live sample (pairs[%d][0] = 0)" % (what, det, det))
        if not np.isfinite(s2[det]).all():
            raise ValueError("%s: detector %d has a non-finite sum: cut non-finite samples with w = 0" % (what, det))
    if normalise == "biased":
        r = s2 / n2[:, 0:1]
    else:
        r = np.where(n2 > 0, s2 / np.maximum(n2, 1), 0.0)
    k = np.arange(lam + 1, dtype=np.float64)
    r = r * (1.0 - k / (lam + 1))
    seq = np.zeros((s2.shape[0], n_fft))
    seq[:, :lam + 1] = r
    seq[:, n_fft - lam:] = r[:, :0:-1]                       # lam = 0: an empty slice on both sides
    psd = np.fft.rfft(seq, axis=-1).real
    low = floor * np.median(psd, axis=-1, keepdims=True)
    if not (low > 0).all():
        raise ValueError("%s: detector %d has a spectrum whose median is not positive" % (what, int(np.flatnonzero(~(low[:, 0] > 0))[0])))
    below = psd < low
    psd = np.where(below, low, psd)
    n_floored = below.sum(axis=-1)
    return (psd[0], int(n_floored[0])) if s.ndim == 1 else (psd, n_floored)


def noise_kernel_from_tod(tod, lam, seg_start=None, w=None, lam_est=None, n_fft=None, normalise="biased", floor=1e-3):
    """The kernel of toeplitz_tod estimated from a timestream of noise, a residual d - P m for instance: the composition
    autocov_tod(tod, lam_est, seg_start, w) -> noise_psd_from_autocov(., n_fft, normalise, floor) -> noise_kernel_from_psd(psd,
    lam), whose arguments these are; lam_est=None is lam.  Returns the (D, lam + 1) Float64 kernel on the device of tod.  The
    autocovariance runs on the device; the two transforms, (D, n_fft) each, on the host."""
    what = "noise_kernel_from_tod"
    lam = _lam(what, lam)
    lam_est = lam if lam_est is None else _lam(what, lam_est)
    sums, pairs = autocov_tod(tod, lam_est, seg_start, w)
    psd, _n_floored = noise_psd_from_autocov(sums, pairs, n_fft, normalise, floor)
    return noise_kernel_from_psd(psd, lam).to(tod.device)


# ---- detector pointing expansion: what produces the skycoords and resp batches of everything above -------------

def quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The Hamilton product a (x) b of (..., 4) quaternion tensors (w, x, y, z), scalar first, broadcasting over the leading
    dimensions.  Plain torch, on whatever device the tensors are: a host-side helper, no kernel."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), dim=-1)


def quat_conj(q: torch.Tensor) -> torch.Tensor:
    """The conjugate (w, -x, -y, -z) of (..., 4) quaternions: the inverse rotation of a unit quaternion."""
    return q * q.new_tensor([1.0, -1.0, -1.0, -1.0])


def quat_from_radec(ra, dec, psi) -> torch.Tensor:
    """The unit quaternion Rz(ra) (x) Ry(pi/2 - dec) (x) Rz(pi - psi), Rz(a) = (cos a/2, 0, 0, sin a/2) and
    Ry(a) = (cos a/2, 0, sin a/2, 0): the rotation that takes z^ to the direction (ra, dec) and x^ to the direction at IAU
    position angle psi there (from north through east).  expand_pointing of it with an identity detector gives back (ra, dec)
    and (cos 2 psi, sin 2 psi).  ra, dec, psi: Float64 tensors (or numbers) that broadcast; returns (..., 4).  A detector that
    looks at (ra_d, dec_d, psi_d) when the boresight is at (ra_b, dec_b, psi_b) has
    q_det = quat_mul(quat_conj(quat_from_radec(ra_b, dec_b, psi_b)), quat_from_radec(ra_d, dec_d, psi_d))."""
    ra, dec, psi = torch.broadcast_tensors(*(torch.as_tensor(v, dtype=torch.float64) for v in (ra, dec, psi)))
    zero = torch.zeros_like(ra)

    def rz(a):
        return torch.stack((torch.cos(a / 2), zero, zero, torch.sin(a / 2)), dim=-1)

    tilt = (math.pi / 2 - dec) / 2
    ry = torch.stack((torch.cos(tilt), zero, torch.sin(tilt), zero), dim=-1)
    return quat_mul(quat_mul(rz(ra), ry), rz(math.pi - psi))


def expand_pointing(q_bore: torch.Tensor, q_det: torch.Tensor, gamma=None, out_sky=None, out_resp=None):
    """Detector pointing expansion (pxl_pointing_expand_f64): (T, 4) boresight quaternions, one per time sample,
    and (D, 4) detector offset quaternions to (skycoords, resp), the (D * T, 2) coordinates (ra, dec) and the (D * T, 2)
    responses gamma_d (cos 2 psi, sin 2 psi) that sample_pol, scatter_pol, normal_pol, bin_pol_nearest and the map-makers take;
    sample k = d * T + t.  Quaternions are (w, x, y, z), R(q) v = q v q*, not necessarily normalised;
    q = q_bore[t] (x) q_det[d] takes z^ to the line of sight and x^ to the polarisation-sensitive direction, whose IAU position
    angle (from north through east) is psi.  ra lies in (-pi, pi]; exactly at a pole ra = +0.0 and east is (0, 1, 0).  gamma: the
    (D,) polarisation efficiencies, None for 1.  A NaN or Inf in a quaternion or gamma, or an all-zero quaternion, makes all four
    outputs of its samples NaN -- a cut sample: the scatters add nothing for it.  out_sky, out_resp: (D * T, 2) buffers to write
    and return instead of new ones; they may not overlap each other or an input.  No atomics: the same inputs give the same
    bits.  Float64, one device."""
    qb = _f64(q_bore, "q_bore", "expand_pointing")
    qd = _on(_f64(q_det, "q_det", "expand_pointing"), "q_det", qb.device)
    if qb.dim() != 2 or qb.shape[1] != 4 or qd.dim() != 2 or qd.shape[1] != 4:
        raise ValueError("q_bore is (T, 4) and q_det is (D, 4): quaternions (w, x, y, z)")
    nt, nd = qb.shape[0], qd.shape[0]
    ins = [qb, qd]
    if gamma is not None:
        g = _on(_f64(gamma, "gamma", "expand_pointing"), "gamma", qb.device)
        if tuple(g.shape) != (nd,):
            raise ValueError("gamma is (D,) with D = %d" % nd)
        ins.append(g)
    outs = []
    for given, name in ((out_sky, "out_sky"), (out_resp, "out_resp")):
        if given is None:
            given = torch.empty((nd * nt, 2), dtype=torch.float64, device=qb.device)
        else:
            _no_f32("expand_pointing", given, name)
            _coords(given, name, qb.device, n=nd * nt)
        if any(_overlap(given, t) for t in ins + outs):
            raise ValueError("out_sky and out_resp may not overlap each other or q_bore, q_det, gamma")
        outs.append(given)
    _call("pxl_pointing_expand_f64", qb, nt, _ptr(qb), nd, _ptr(qd), None if gamma is None else _ptr(ins[2]), _ptr(outs[0]), _ptr(outs[1]))
    return outs[0], outs[1]


# ---- synthetic inputs (benchmark plumbing) --------------------------------------------------------

def fill_random_(t: torch.Tensor, seed: int, offset: int = 0, kind: str = "normal"):
    t = _dev_f64(t, "tensor")
    _call("pxl_fill_random_f64", t, _ptr(t), t.numel(), seed, offset, 0 if kind == "normal" else 1)
    return t


def fill_sphere_points_(sky: torch.Tensor, seed: int, offset: int = 0):
    sky = _coords(sky, "skycoords")
    _call("pxl_fill_sphere_points_f64", sky, _ptr(sky), sky.shape[0], seed, offset)
    return sky
