"""Position-velocity diagrams on the device: the spectrum of the filled cube at every point of a path drawn on the sky,
``(nz, npts)``.  Stands in for ``SpectralCube.to_pvextractor()`` + ``pvextractor.extract_pv_slice(cube, path)``
(spectral_cube.py:2506-2513) and for the axis-aligned ``cube[:, j, :]``; the cube never leaves HBM, only the diagram comes
down (ops.pv_extract, spc_pv_extract_f32 / _f64).

    path = Path([(12.0, 40.5), (200.0, 150.0), (310.0, 150.0)], width=5)       # pixel positions (x, y), width in pixels
    pv = extract_pv_slice(cube, path, spacing=1.0)                              # a Projection of shape (nz, npts)
    pv = cube.pv_slice(Path.from_world(lon, lat, cube.wcs))                     # the same through the cube
    row = cube.pv_slice(y=40)                                                   # filled_data[:, 40, :], bit for bit

Two deliberate deviations from pvextractor:

* the default is ``order=1`` (bilinear), not pvextractor's 3.  Orders 2 / 3 raise NotImplementedError: a B-spline
  prefilter runs over whole planes, scipy turns one NaN into an all-NaN plane, and the spline resampler of ``reproject``
  uses another edge convention ([-0.5, n - 0.5] on replicated borders).  Smooth the cube first, or use ``order=1``.
* a path with a *width* is the mean of ``nlines`` parallel interpolated lines (NaN samples left out), not pvextractor's
  area-weighted polygons.

Sampling is the kernel's rule (include/spcube_hip.h): a point is inside when ``0 <= x <= nx - 1`` and ``0 <= y <= ny - 1``
and NaN otherwise (scipy.ndimage.map_coordinates with ``mode='constant', cval=nan``); samples are the cube's FILLED values.
"""
import math

import numpy as np

from . import ops

__all__ = ["Path", "extract_pv_slice"]


class Path:
    """A polyline on the sky in 0-based pixel coordinates: *points* a sequence of ``(x, y)``, *width* the full width in
    pixels over which parallel lines are averaged (None: the line alone).  Zero-length segments and a path of fewer than
    two distinct points raise ValueError."""

    def __init__(self, points, width=None):
        pts = np.array(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("points must be a sequence of (x, y) pixel positions (got an array of shape %s)" % (pts.shape,))
        if not np.all(np.isfinite(pts)):
            raise ValueError("every point of a path must be finite")
        if len(pts) < 2:
            raise ValueError("a path needs at least two distinct points (got %d)" % len(pts))
        seg = np.hypot(*(pts[1:] - pts[:-1]).T)
        if np.any(seg == 0.0):
            raise ValueError("segment %d of the path has zero length: drop the repeated point" % int(np.argmax(seg == 0.0)))
        if width is not None:
            width = float(width)
            if not (width >= 0.0 and math.isfinite(width)):
                raise ValueError("width must be a finite number of pixels >= 0 (got %r)" % (width,))
        self.points = pts
        self.width = width
        self._seg = seg
        self._cum = np.concatenate(([0.0], np.cumsum(seg)))

    @classmethod
    def from_world(cls, lon_deg, lat_deg, wcs, width=None):
        """the path through the sky positions (*lon_deg*, *lat_deg*) (degrees, sequences of one length) in the pixels of
        *wcs* (SimpleWCS.celestial_world2pix); *width* stays in pixels"""
        px, py = wcs.celestial_world2pix(np.asarray(lon_deg, dtype=np.float64), np.asarray(lat_deg, dtype=np.float64))
        return cls(np.stack([np.atleast_1d(px), np.atleast_1d(py)], axis=1), width=width)

    @property
    def length(self):
        return float(self._cum[-1])

    def _sample(self, spacing):
        """(points (npts, 2), segment index per point): arc lengths k * spacing, k = 0 ... floor(L / spacing + 1e-9)"""
        spacing = float(spacing)
        if not (spacing > 0.0 and math.isfinite(spacing)):
            raise ValueError("spacing must be a positive number of pixels (got %r)" % (spacing,))
        npts = int(math.floor(self.length / spacing + 1e-9)) + 1
        s = np.minimum(np.arange(npts, dtype=np.float64) * spacing, self.length)
        # the segment holding the point: at a vertex the following one, at the last point the last one
        i = np.clip(np.searchsorted(self._cum, s, side="right") - 1, 0, len(self._seg) - 1)
        t = (s - self._cum[i]) / self._seg[i]
        a, b = self.points[i], self.points[i + 1]
        return a + t[:, None] * (b - a), i

    def sample_points(self, spacing=1.0):
        """(npts, 2) float64 positions (x, y) at arc lengths ``k * spacing`` along the polyline, linearly between vertices"""
        return self._sample(spacing)[0]

    def sample_lines(self, spacing=1.0, nlines=None):
        """(xs, ys), each (nlines, npts) float64: line ``l`` is the sampled path moved by ``((l + 0.5) / nlines - 0.5) * width``
        along the local normal ``(-dy, dx) / |d|``, d the direction of the segment holding the point (at a vertex the
        following segment, at the last point the last one).  *nlines* defaults to ``max(1, ceil(width))``."""
        pts, i = self._sample(spacing)
        width = 0.0 if self.width is None else self.width
        if nlines is None:
            nlines = max(1, int(math.ceil(width)))
        if int(nlines) != nlines or nlines < 1:
            raise ValueError("nlines must be an integer >= 1 (got %r)" % (nlines,))
        nlines = int(nlines)
        d = (self.points[i + 1] - self.points[i]) / self._seg[i][:, None]
        normal = np.stack([-d[:, 1], d[:, 0]], axis=1)
        off = ((np.arange(nlines, dtype=np.float64) + 0.5) / nlines - 0.5) * width
        xs = pts[None, :, 0] + off[:, None] * normal[None, :, 0]
        ys = pts[None, :, 1] + off[:, None] * normal[None, :, 1]
        return np.ascontiguousarray(xs), np.ascontiguousarray(ys)


def _check_order(order):
    if order in (2, 3):
        raise NotImplementedError(
            "order %d is not built: a B-spline prefilter runs over whole planes and turns one NaN into an all-NaN plane; "
            "use order=1 (bilinear, the default here - pvextractor's is 3) or order=0, after smoothing the cube if needed" % order)
    if order not in (0, 1):
        raise ValueError("order must be 0 (nearest) or 1 (bilinear) (got %r)" % (order,))
    return int(order)


def pv_header(cube, npts, spacing):
    """the header of a diagram of *npts* points *spacing* pixels apart: axis 1 the offset along the path in the celestial
    unit (pvextractor's convention: spacing x sqrt|det pixel_scale_matrix|), axis 2 the cube's spectral axis; {} without a WCS"""
    w = cube.wcs
    if w is None:
        return {}
    psm = np.asarray(w.pixel_scale_matrix)[:2, :2]
    scale = math.sqrt(abs(psm[0, 0] * psm[1, 1] - psm[0, 1] * psm[1, 0]))
    h = {"NAXIS": 2, "NAXIS1": int(npts), "NAXIS2": int(cube.shape[0]), "WCSAXES": 2,
         "CTYPE1": "OFFSET", "CRPIX1": 1.0, "CRVAL1": 0.0, "CDELT1": float(spacing) * scale, "CUNIT1": w.cunit[0]}
    if w.naxis >= 3:
        h.update({"CTYPE2": w.ctype[2], "CRVAL2": float(w.crval[2]), "CDELT2": float(w.cdelt[2] * w.pc[2, 2]),
                  "CRPIX2": float(w.crpix[2]), "CUNIT2": w.cunit[2]})
        if "RESTFRQ" in w.header:
            h["RESTFRQ"] = w.header["RESTFRQ"]
    if cube.unit:
        h["BUNIT"] = cube.unit
    return h


def _extract(cube, xs, ys, order, respect_nan, spacing, meta):
    """the Projection of the diagram at the pixel positions *xs*, *ys* ((nlines, npts) float64)"""
    from .cube import Projection, VaryingResolutionSpectralCube, _nan_term_dropped
    if cube._stream_source() is not None:
        raise NotImplementedError(
            "a position-velocity diagram needs the cube in HBM and this one is larger than the budget (SPC_HBM_BUDGET): cut "
            "it first - cube[:, y0:y1, x0:x1] or spectral_slab() around the path stream only what they touch - and extract "
            "from the cut")
    data, mspec, view = cube._operand()
    has_mask = cube._mask is not None
    out = ops.pv_extract(data, xs, ys, order=order, respect_nan=respect_nan, mask_spec=mspec if has_mask else None,
                         fill=cube._fill_value, nan_excluded=_nan_term_dropped(cube, view))
    varying = isinstance(cube, VaryingResolutionSpectralCube)
    full = dict(cube.meta)
    if varying:
        full.pop("beam", None)
    full.update(meta)
    return Projection(out.get(), unit=cube.unit, wcs=None, meta=full, beam=None if varying else cube.beam, device=cube.device,
                      header=pv_header(cube, xs.shape[-1], spacing))


def extract_pv_slice(cube, path, spacing=1.0, order=1, respect_nan=True, nlines=None):
    """The position-velocity diagram of *cube* along *path* (a :class:`Path` or a plain list of ``(x, y)`` pixel positions),
    one point every *spacing* pixels: a Projection of shape ``(nz, npts)`` in the cube's unit and dtype, computed on the
    device from the cube's filled data (pvextractor.extract_pv_slice; spectral_cube.py:2506-2513).

    *order*: 1 (bilinear, the default) or 0 (nearest).  NOT pvextractor's default of 3: orders 2 / 3 raise
    NotImplementedError (see the module docstring).  *respect_nan*: a NaN under the interpolation footprint makes the sample
    NaN; otherwise it counts as 0.  A path with a width is the mean of *nlines* (default ``max(1, ceil(width))``) parallel
    lines, NaN samples left out - not pvextractor's area-weighted polygons.  Points outside the plane are NaN.

    ``meta`` records ``pv_path``, ``pv_spacing``, ``pv_width``, ``pv_order``; the header's axis 1 is ``OFFSET`` along the
    path (CDELT1 = spacing x the pixel scale, in the celestial unit), axis 2 the cube's spectral axis.  Without a WCS there
    is no header and the offset is in pixels.  A VaryingResolutionSpectralCube gives ``beam=None``.  A cube larger than
    the HBM budget raises NotImplementedError."""
    order = _check_order(order)
    if not isinstance(path, Path):
        path = Path(path)
    xs, ys = path.sample_lines(spacing, nlines)
    meta = {"pv_path": [tuple(float(v) for v in p) for p in path.points], "pv_spacing": float(spacing),
            "pv_width": path.width, "pv_order": order}
    return _extract(cube, xs, ys, order, respect_nan, float(spacing), meta)


def axis_cut(cube, y=None, x=None):
    """``cube.pv_slice(y=j)`` / ``pv_slice(x=i)``: one order-0 line along the row / column, an exact copy of
    ``filled_data[:, j, :]`` / ``filled_data[:, :, i]``; negative indices as in numpy"""
    if (y is None) == (x is None):
        raise ValueError("give exactly one of y= (a row) and x= (a column)")
    nz, ny, nx = cube.shape
    axis, n, k = ("y", ny, y) if y is not None else ("x", nx, x)
    if int(k) != k:
        raise TypeError("%s must be an integer index (got %r)" % (axis, k))
    k = int(k)
    if not -n <= k < n:
        raise IndexError("index %d is out of bounds for the %s axis of a cube of shape %s" % (k, axis, cube.shape))
    k += n if k < 0 else 0
    if y is not None:
        xs, ys = np.arange(nx, dtype=np.float64), np.full(nx, float(k))
        ends = [(0.0, float(k)), (float(nx - 1), float(k))]
    else:
        xs, ys = np.full(ny, float(k)), np.arange(ny, dtype=np.float64)
        ends = [(float(k), 0.0), (float(k), float(ny - 1))]
    meta = {"pv_path": ends, "pv_spacing": 1.0, "pv_width": None, "pv_order": 0}
    return _extract(cube, xs[None], ys[None], 0, True, 1.0, meta)
