"""CPU oracle: numpy float64 restatement of spectral-cube's dense hot path.

TEST INFRASTRUCTURE ONLY.  Only ``tests/``, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of ``bench.py`` may import this module; the product path
(``spectral_cube_amd``) never does and fails loudly when the HIP library is
missing.

Every function cites the reference lines it restates (paths relative to
``/root/reference``).  Parity is PINNED for moments / argmax / spectral_smooth /
spatial_smooth / spectral_interpolate: ``oracle/gen_golden.py`` runs the real
reference (imported via ``oracle/ref_env/bootstrap.py``) and asserts these
functions reproduce it, and ``tests/test_oracle_golden.py`` re-checks them
against the committed vectors in ``tests/golden/`` plus the reference's own
hand-written golden tables (spectral_cube/tests/test_moments.py:19-49 etc.).
``resample_bilinear``: the reference delegates to the third-party ``reproject``
package (neither vendored nor installed; the reference's tests never check its
pixel values - SURVEY.md section 8c).  Its bilinear resampler is
``scipy.ndimage.map_coordinates(order=1)`` on the edge-padded image; the
restatement is pinned against THAT with the scipy installed here
(``gen_golden.case_bilinear_scipy`` -> tests/golden/bilinear_scipy.npz).  The
celestial pixel map itself is pinned against astropy.wcs (wcs.npz).

Array layout everywhere: C-contiguous ``(nz, ny, nx)``, spectral axis first.
"""
import numpy as np

__all__ = [
    "filled", "moment", "moments012", "moment_cubewise", "argmax", "argmin",
    "convolve_fill_interp", "spectral_smooth", "spatial_smooth",
    "spectral_interpolate", "resample_bilinear", "reproject_separable",
    "statistics", "reduce", "fits_decode", "median", "percentile", "mad_std", "sigma_clip",
    "beam_second_moments", "beam_from_second_moments", "deconvolve_beam", "elliptical_gaussian_kernel",
]


# --------------------------------------------------------------------------
# mask -> filled data
# --------------------------------------------------------------------------
def filled(data, include=None, fill=np.nan):
    """``MaskBase._filled`` (spectral_cube/masks.py:197-237).

    ``data.astype(result_type(dtype, 0.0))`` with excluded voxels replaced by
    *fill*; ``include=None`` means "no mask" (base_class.py:389-417 returns the
    raw data then).  The dtype is kept (fp32 stays fp32).
    """
    dt = np.result_type(data.dtype, 0.0)
    out = np.array(data, dtype=dt, copy=True)
    if include is not None:
        out[~np.asarray(include, dtype=bool)] = fill
    return out


def _nansum_allbadtonan(a, axis):
    """``allbadtonan(np.nansum)`` (spectral_cube/np_compat.py:3-27)."""
    res = np.nansum(a, axis=axis)
    allbad = np.all(np.isnan(a), axis=axis)
    res = np.asarray(res, dtype=a.dtype)
    res[allbad] = np.nan
    return res


# --------------------------------------------------------------------------
# moments
# --------------------------------------------------------------------------
def _bcast_cen(pix_cen, shape, axis):
    """pix_cen may be 1-D along *axis* (spectral) or a full/broadcastable 3-D
    array (spatial axes, spectral_cube.py:1455-1508)."""
    pix_cen = np.asarray(pix_cen, dtype=np.float64)
    if pix_cen.ndim == 1:
        shp = [1, 1, 1]
        shp[axis] = shape[axis]
        pix_cen = pix_cen.reshape(shp)
    return pix_cen


def moment(data, include, order, pix_cen, pix_size, axis=0, world0=None):
    """``DaskSpectralCubeMixin.moment`` arithmetic
    (spectral_cube/dask_spectral_cube.py:1083-1123), evaluated eagerly.

    data     fp32/fp64 cube, include bool mask or None
    pix_cen  offsets from pixel 0 along *axis* (spectral_cube.py:1473-1475)
    pix_size scalar pixel size along *axis* (spectral_cube.py:1510-1535)
    world0   added to moment 1 when axis == 0 (dask_spectral_cube.py:1122-1123)
    Returns float64.
    """
    d = filled(data, include, np.nan).astype(np.float64)        # :1083
    cen = _bcast_cen(pix_cen, d.shape, axis)
    if order == 0:
        return _nansum_allbadtonan(d * pix_size, axis)           # :1087-1088
    denominator = _nansum_allbadtonan(d * pix_size, axis)       # :1090
    with np.errstate(invalid="ignore", divide="ignore"):
        mom1 = _nansum_allbadtonan(d * pix_size * cen, axis) / denominator
        if order > 1:
            mom1k = np.expand_dims(mom1, axis)                  # :1094-1097
            out = (_nansum_allbadtonan(d * pix_size * (cen - mom1k) ** order,
                                       axis) / denominator)     # :1098-1099
        else:
            out = mom1
    if order == 1 and axis == 0 and world0 is not None:
        out = out + world0                                      # :1122-1123
    return out


def moments012(data, include, pix_cen, pix_size, world0=0.0):
    """moment 0, 1, 2 along axis 0 in one call (three reference passes)."""
    return (moment(data, include, 0, pix_cen, pix_size),
            moment(data, include, 1, pix_cen, pix_size, world0=world0),
            moment(data, include, 2, pix_cen, pix_size))


def moment_cubewise(data, include, order, pix_cen, pix_size, axis=0):
    """``moment_cubewise`` (spectral_cube/_moments.py:170-193): NumPy-class
    strategy.  Only moment 0 maps all-bad rays to NaN explicitly; orders >= 1
    get NaN from 0/0.  Computed in float64 here (numpy >= 2 promotion)."""
    d = filled(data, include, np.nan).astype(np.float64) * pix_size
    cen = _bcast_cen(pix_cen, d.shape, axis)
    if order == 0:
        return _nansum_allbadtonan(d, axis)
    with np.errstate(invalid="ignore", divide="ignore"):
        if order == 1:
            return np.nansum(d * cen, axis=axis) / np.nansum(d, axis=axis)
        mom1 = np.expand_dims(moment_cubewise(data, include, 1, pix_cen,
                                              pix_size, axis), axis)
        return (np.nansum(d * (cen - mom1) ** order, axis=axis) /
                np.nansum(d, axis=axis))


# --------------------------------------------------------------------------
# argmax / argmin  (integer maps: bit-exact)
# --------------------------------------------------------------------------
def _arg(data, include, axis, fill, fn):
    d = filled(data, include, fill)
    # np.nanarg* raise on all-NaN rays; the reference's rays are filled with
    # +-inf where masked, so only NaN *data* inside the mask can trigger that.
    # Treat NaN as the fill value (what nanargmax does for partial NaN rays).
    d = np.where(np.isnan(d), fill, d)
    return fn(d, axis=axis).astype(np.int64)


def argmax(data, include=None, axis=0):
    """``argmax`` (spectral_cube/spectral_cube.py:793-804;
    dask_spectral_cube.py:749-757): nanargmax of data filled with -inf.
    First index wins ties; a fully masked ray gives 0."""
    return _arg(data, include, axis, -np.inf, np.argmax)


def argmin(data, include=None, axis=0):
    """``argmin`` (spectral_cube/spectral_cube.py:806-819): fill +inf."""
    return _arg(data, include, axis, np.inf, np.argmin)


# --------------------------------------------------------------------------
# astropy.convolution.convolve semantics (third-party; astropy>=6.1 declared
# in pyproject.toml:26, 4.3.1 probed here).  Call sites:
# dask_spectral_cube.py:912-914, 990-993; spectral_cube.py:2833-2837, 3216-3222
# --------------------------------------------------------------------------
def convolve_fill_interp(array, kernel, normalize_kernel=True):
    """``astropy.convolution.convolve(array, kernel, boundary='fill',
    fill_value=0, nan_treatment='interpolate', normalize_kernel=True)``.

    * true convolution (kernel flipped), direct sum, float64 internally;
    * out-of-bounds samples are *valid zeros* (they contribute to the weight
      sum);
    * if the array contains any NaN: ``out = sum(k*d over non-NaN) /
      sum(k over non-NaN)``, and where that weight sum is 0 the (NaN) centre
      sample is returned; otherwise ``out = sum(k*d) / sum(k)``;
    * result cast back to the input floating dtype.
    """
    array = np.asarray(array)
    kernel = np.asarray(kernel, dtype=np.float64)
    if array.ndim != kernel.ndim:
        raise ValueError("array and kernel have differing number of dimensions")
    if any(s % 2 == 0 for s in kernel.shape):
        raise ValueError("kernel axes must be odd")
    a = array.astype(np.float64)
    pad = [s // 2 for s in kernel.shape]
    ap = np.pad(a, [(p, p) for p in pad], mode="constant", constant_values=0.0)
    isn = np.isnan(ap)
    any_nan = bool(isn.any())
    v = np.where(isn, 0.0, ap)
    w = (~isn).astype(np.float64)
    top = np.zeros(a.shape, dtype=np.float64)
    bot = np.zeros(a.shape, dtype=np.float64)
    kflip = kernel[tuple(slice(None, None, -1) for _ in kernel.shape)]
    for idx in np.ndindex(*kernel.shape):
        kv = kflip[idx]
        if kv == 0.0:
            continue
        sl = tuple(slice(i, i + n) for i, n in zip(idx, a.shape))
        top += kv * v[sl]
        if any_nan:
            bot += kv * w[sl]
    ksum = kernel.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        if any_nan:
            res = np.where(bot != 0.0, top / np.where(bot != 0.0, bot, 1.0), a)
            if not normalize_kernel:
                res = res * ksum
        else:
            res = top / ksum if normalize_kernel else top
    if array.dtype.kind == "f":
        res = res.astype(array.dtype)
    return res


def spectral_smooth(data, include, kernel1d, fill=np.nan):
    """``DaskSpectralCubeMixin.spectral_smooth``
    (dask_spectral_cube.py:880-917): convolve the NaN-filled chunk with the
    kernel reshaped to (n,1,1).  The returned cube keeps the ORIGINAL mask
    (dask_spectral_cube.py:836-840) - callers re-apply *include* themselves.
    NaN-awareness is decided per chunk by astropy; the whole cube is one chunk
    here, which is numerically equivalent (the two branches agree when no NaN
    is present up to rounding)."""
    d = filled(data, include, fill)
    k = np.asarray(kernel1d, dtype=np.float64).reshape(-1, 1, 1)
    return convolve_fill_interp(d, k)


def spatial_smooth(data, include, kernel2d, fill=np.nan):
    """``DaskSpectralCubeMixin.spatial_smooth``
    (dask_spectral_cube.py:962-993 + wrapper :540-547): every channel is
    convolved independently with the 2-D kernel."""
    d = filled(data, include, fill)
    k = np.asarray(kernel2d, dtype=np.float64)
    out = np.empty_like(d)
    for i in range(d.shape[0]):
        out[i] = convolve_fill_interp(d[i], k)
    return out


# --------------------------------------------------------------------------
# spectral_interpolate  (Dask semantics, scipy.interpolate.interp1d linear)
# --------------------------------------------------------------------------
def spectral_interpolate(data, include, inaxis, grid, fill_value=None,
                         out_dtype=None):
    """``DaskSpectralCubeMixin.spectral_interpolate``
    (dask_spectral_cube.py:1291-1373) with scipy ``interp1d(kind='linear',
    bounds_error=False, fill_value=fill_value)`` restated
    (scipy/interpolate/_interpolate.py ``_call_linear`` + ``_check_bounds``;
    scipy>=1.8.1 declared in pyproject.toml:52).

    inaxis / grid: spectral coordinates (same unit) of the input channels and
    of the requested output channels; either may be descending.  Output
    channel order follows *grid* as given (dask_spectral_cube.py:1366-1367).
    Returns (newdata, newmask) with newmask = ~isnan(newdata) (:1364).
    """
    inaxis = np.asarray(inaxis, dtype=np.float64)
    grid = np.asarray(grid, dtype=np.float64)
    d = filled(data, include, np.nan)
    reverse_in = np.mean(np.diff(inaxis)) < 0                  # :1293-1304
    reverse_out = np.mean(np.diff(grid)) < 0
    if reverse_in:
        inaxis = inaxis[::-1]
        d = d[::-1]
    if reverse_out:
        grid = grid[::-1]
    if not (np.all(np.diff(grid) > 0) and np.all(np.diff(inaxis) > 0)):
        raise AssertionError("axes must be monotonic")           # :1315-1316
    np.testing.assert_allclose(np.diff(grid), np.mean(np.diff(grid)),
                               err_msg="Output grid must be linear")  # :1318
    idx = np.searchsorted(inaxis, grid)
    idx = np.clip(idx, 1, len(inaxis) - 1).astype(int)
    lo, hi = idx - 1, idx
    x_lo, x_hi = inaxis[lo], inaxis[hi]
    y_lo, y_hi = d[lo], d[hi]
    with np.errstate(invalid="ignore"):
        slope = (y_hi - y_lo) / (x_hi - x_lo)[:, None, None]
        y_new = slope * (grid - x_lo)[:, None, None] + y_lo
    oob = (grid < inaxis[0]) | (grid > inaxis[-1])
    y_new = np.asarray(y_new, dtype=np.float64)
    y_new[oob] = np.nan if fill_value is None else fill_value
    newmask = ~np.isnan(y_new)
    if reverse_out:
        y_new = y_new[::-1]
        newmask = newmask[::-1]
    if out_dtype is not None:
        y_new = y_new.astype(out_dtype)
    return y_new, newmask


# --------------------------------------------------------------------------
# reprojection (pinned against scipy's map_coordinates - see module docstring)
# --------------------------------------------------------------------------
def resample_bilinear(plane_or_cube, xs, ys):
    """Bilinear resampling of every channel at source pixel coordinates
    ``(xs, ys)`` (0-based, pixel centres at integers): the resampler behind
    ``reproject.reproject_interp(order='bilinear')`` (call site
    spectral_cube/spectral_cube.py:2726-2732).  reproject itself is not in this
    image; its resampler is published as: pad the image by one edge-replicated
    pixel, ``scipy.ndimage.map_coordinates(padded, coords + 1, order=1,
    mode='constant', cval=nan)``, then reset every output whose source
    position lies outside ``[-0.5, n - 0.5]`` to NaN (footprint 0).  This
    restates exactly that, and oracle/gen_golden.py pins it against
    scipy.ndimage.map_coordinates (tests/golden/bilinear_scipy.npz).
    Consequences reproduced here: a NaN neighbour propagates even with weight 0
    (exact hits next to a NaN are NaN); within half a pixel of the border both
    neighbours are the border pixel.
    Returns (data, footprint)."""
    a = np.asarray(plane_or_cube)
    cube = a if a.ndim == 3 else a[None]
    nz, ny, nx = cube.shape
    xs = np.asarray(xs, dtype=np.float64)
    ys = np.asarray(ys, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = ((xs >= -0.5) & (xs <= nx - 0.5) &
                  (ys >= -0.5) & (ys <= ny - 0.5))
    inside &= np.isfinite(xs) & np.isfinite(ys)
    xq = np.where(inside, xs, 0.0)
    yq = np.where(inside, ys, 0.0)
    xf = np.floor(xq)
    yf = np.floor(yq)
    fx = xq - xf                                   # weight of the upper neighbour, in [0, 1)
    fy = yq - yf
    x0 = xf.astype(np.int64)                       # in [-1, nx - 1]: -1 / nx are the replicated border
    y0 = yf.astype(np.int64)
    xa, xb = np.maximum(x0, 0), np.minimum(x0 + 1, nx - 1)
    ya, yb = np.maximum(y0, 0), np.minimum(y0 + 1, ny - 1)
    out = np.empty((nz,) + xs.shape, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for k in range(nz):
            p = cube[k].astype(np.float64)
            v = (p[ya, xa] * ((1 - fy) * (1 - fx)) + p[ya, xb] * ((1 - fy) * fx) +
                 p[yb, xa] * (fy * (1 - fx)) + p[yb, xb] * (fy * fx))
            out[k] = np.where(inside, v, np.nan)
    foot = np.broadcast_to(inside, out.shape).copy()
    if a.ndim == 2:
        return out[0], foot[0]
    return out, foot


def resample_nearest(plane_or_cube, xs, ys):
    """``reproject_interp(order='nearest-neighbor')``: the same published steps as resample_bilinear
    with ``scipy.ndimage.map_coordinates(..., order=0)`` - the sample whose centre is nearest
    (``floor(x + 0.5)``; inside the half-pixel border zone that is the border pixel), no neighbour
    takes part, so a NaN only shows where it is picked.  Pinned against scipy in
    oracle/gen_golden.py (tests/golden/reproject_glue_scipy.npz).  Returns (data, footprint)."""
    a = np.asarray(plane_or_cube)
    cube = a if a.ndim == 3 else a[None]
    nz, ny, nx = cube.shape
    xs = np.asarray(xs, dtype=np.float64)
    ys = np.asarray(ys, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = ((xs >= -0.5) & (xs <= nx - 0.5) & (ys >= -0.5) & (ys <= ny - 0.5))
    inside &= np.isfinite(xs) & np.isfinite(ys)
    xi = np.clip(np.floor(np.where(inside, xs, 0.0) + 0.5).astype(np.int64), 0, nx - 1)
    yi = np.clip(np.floor(np.where(inside, ys, 0.0) + 0.5).astype(np.int64), 0, ny - 1)
    out = np.where(inside[None], cube[:, yi, xi].astype(np.float64), np.nan)
    foot = np.broadcast_to(inside, out.shape).copy()
    if a.ndim == 2:
        return out[0], foot[0]
    return out, foot


def _spline_pole(order):
    """the single pole of the B-spline prefilter of degree 2 / 3 (scipy ndimage ni_splines.c get_filter_poles)"""
    if order == 2:
        return np.sqrt(8.0) - 3.0
    if order == 3:
        return np.sqrt(3.0) - 2.0
    raise ValueError("spline order 2 or 3")


def spline_prefilter_axis(a, order, axis):
    """B-spline coefficients of the samples along one axis with MIRROR boundaries, float64: the recursive filter of
    ``scipy.ndimage.spline_filter1d`` (ni_splines.c: gain, _init_causal_mirror, the causal / anticausal recursions,
    _init_anticausal_mirror) - what ``map_coordinates(prefilter=True, mode='constant')`` runs along every axis (for that
    mode scipy filters with the mirror boundary).  A line of one sample is left alone, like scipy."""
    a = np.moveaxis(np.array(a, dtype=np.float64, copy=True), axis, 0)
    n = a.shape[0]
    if n < 2:
        return np.moveaxis(a, 0, axis)
    z = _spline_pole(order)
    a *= (1.0 - z) * (1.0 - 1.0 / z)
    z_n_1 = z ** (n - 1)
    c0 = a[0] + z_n_1 * a[n - 1]
    z_i = z
    for i in range(1, n - 1):
        c0 = c0 + z_i * (a[i] + z_n_1 * a[n - 1 - i])
        z_i *= z
    a[0] = c0 / (1.0 - z_n_1 * z_n_1)
    for i in range(1, n):
        a[i] += z * a[i - 1]
    a[n - 1] = (z * a[n - 2] + a[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        a[i] = z * (a[i + 1] - a[i])
    return np.moveaxis(a, 0, axis)


def _spline_weights(x, order):
    """(first support index, weights) of scipy's get_spline_interpolation_weights for coordinates x"""
    if order == 3:
        f = np.floor(x)
        y = x - f
        zz = 1.0 - y
        w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
        w2 = (zz * zz * (zz - 2.0) * 3.0 + 4.0) / 6.0
        w0 = zz * zz * zz / 6.0
        return f.astype(np.int64) - 1, [w0, w1, w2, 1.0 - w0 - w1 - w2]
    f = np.floor(x + 0.5)
    y = x - f
    w1 = 0.75 - y * y
    t = 0.5 - y
    w0 = 0.5 * t * t
    return f.astype(np.int64) - 1, [w0, w1, 1.0 - w0 - w1]


def resample_spline(plane_or_cube, xs, ys, order):
    """``reproject_interp(order='biquadratic' | 'bicubic')`` (the orders ``BaseSpectralCube.reproject`` documents,
    spectral_cube.py:2667-2676) for a cube whose channels map onto themselves: reproject's published steps - replicate the
    border by one pixel, ``scipy.ndimage.map_coordinates(order=2 | 3, mode='constant', cval=nan)`` at coordinates + 1, NaN
    where a coordinate is outside [-0.5, n - 0.5] - with scipy's spline arithmetic restated: mirror-boundary prefilter along
    y and x (along z the filter is undone exactly by sampling at integer channels), mirror-folded support indices.
    A non-finite sample ANYWHERE in the cube makes scipy's recursive prefilter (which runs along z too) return NaN
    everywhere: so does this.  Pinned against scipy in oracle/gen_golden.py (tests/golden/reproject_spline_scipy.npz).
    Returns (data, footprint)."""
    a = np.asarray(plane_or_cube)
    cube = a if a.ndim == 3 else a[None]
    nz, ny, nx = cube.shape
    xs = np.asarray(xs, dtype=np.float64)
    ys = np.asarray(ys, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = ((xs >= -0.5) & (xs <= nx - 0.5) & (ys >= -0.5) & (ys <= ny - 0.5))
    inside &= np.isfinite(xs) & np.isfinite(ys)
    out = np.full((nz,) + xs.shape, np.nan)
    if np.isfinite(cube).all():
        xq, yq = np.where(inside, xs, 0.0) + 1.0, np.where(inside, ys, 0.0) + 1.0
        ix, wx = _spline_weights(xq, order)
        iy, wy = _spline_weights(yq, order)

        def fold(i, n):                       # mirror about the first / last sample
            i = np.abs(i)
            return np.where(i > n - 1, 2 * (n - 1) - i, i)
        for k in range(nz):
            c = np.pad(cube[k].astype(np.float64), 1, mode="edge")
            c = spline_prefilter_axis(spline_prefilter_axis(c, order, 0), order, 1)
            v = np.zeros(xs.shape)
            for j, wyj in enumerate(wy):
                yy = fold(iy + j, ny + 2)
                for i, wxi in enumerate(wx):
                    v = v + wyj * wxi * c[yy, fold(ix + i, nx + 2)]
            out[k] = np.where(inside, v, np.nan)
    foot = np.broadcast_to(inside, out.shape).copy()
    if a.ndim == 2:
        return out[0], foot[0]
    return out, foot


def reproject_separable(cube, xs, ys, zs=None):
    """Spatial bilinear resample, optionally composed with a linear resample
    along z at fractional channel positions *zs* (trilinear with a separable
    coordinate map: what reproject_interp does for cube headers whose spectral
    and celestial axes are independent)."""
    out, foot = resample_bilinear(cube, xs, ys)
    if zs is None:
        return out, foot
    nz = out.shape[0]
    zs = np.asarray(zs, dtype=np.float64)
    inside = (zs >= -0.5) & (zs <= nz - 0.5)
    zc = np.clip(np.where(inside, zs, 0.0), 0.0, nz - 1.0)
    z0 = np.minimum(np.floor(zc).astype(np.int64), max(nz - 2, 0))
    z1 = np.minimum(z0 + 1, nz - 1)
    fz = (zc - z0)[:, None, None]
    res = (1 - fz) * out[z0] + fz * out[z1]
    res[~inside] = np.nan
    f = foot[z0] & foot[z1] & inside[:, None, None]
    return res, f


# --------------------------------------------------------------------------
# statistics / nan-reductions
# --------------------------------------------------------------------------
def statistics(data, include=None):
    """``DaskSpectralCubeMixin.statistics`` (spectral_cube/dask_spectral_cube.py:
    769-814): npts / min / max / sum / sumsq of the NaN-filled data, then
    ``mean = sum/npts``, the reference's "textbook" ``sigma = sqrt((sumsq -
    sum**2/npts) / (npts - 1))`` and ``rms = sqrt(sumsq/npts)``.  The reference
    sums each chunk in the chunk dtype (float32 pairwise) before aggregating in
    float64; this restatement sums in float64 throughout, so it agrees with the
    reference to float32 summation accuracy (gen_golden asserts rtol 2e-6)."""
    d = filled(data, include, np.nan).astype(np.float64)
    ok = ~np.isnan(d)
    npts = float(ok.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        st = {"npts": npts,
              "min": float(np.min(d[ok])) if npts else np.nan,
              "max": float(np.max(d[ok])) if npts else np.nan,
              "sum": float(np.sum(d[ok])),
              "sumsq": float(np.sum(d[ok] * d[ok]))}
        st["mean"] = st["sum"] / npts if npts else np.nan
        st["sigma"] = (((st["sumsq"] - st["sum"] ** 2 / npts) / (npts - 1)) ** 0.5
                       if npts > 1 else np.nan)
        st["rms"] = np.sqrt(st["sumsq"] / npts) if npts else np.nan
    return st


def reduce(data, include, op, axis=None, ddof=0):
    """``sum`` / ``mean`` / ``std`` / ``max`` / ``min`` of the Dask class
    (spectral_cube/dask_spectral_cube.py:641-767): nansum_allbadtonan, nanmean,
    nanstd(ddof), nanmax, nanmin of the NaN-filled data; rays (or a cube)
    without valid samples give NaN.  float64."""
    import warnings
    d = filled(data, include, np.nan).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if op == "sum":
            if axis is None:
                return np.nan if np.all(np.isnan(d)) else float(np.nansum(d))
            return _nansum_allbadtonan(d, axis)
        if op == "mean":
            return np.nanmean(d, axis=axis)
        if op == "std":
            return np.nanstd(d, axis=axis, ddof=ddof)
        if op == "max":
            return np.nanmax(d, axis=axis) if d.size else np.nan
        if op == "min":
            return np.nanmin(d, axis=axis) if d.size else np.nan
    raise ValueError(op)


# --------------------------------------------------------------------------
# FITS payload decoding
# --------------------------------------------------------------------------
def fits_decode(raw, bitpix, shape, bscale=1.0, bzero=0.0, blank=None, out_dtype=np.float32, astropy_quirks=False):
    """What ``astropy.io.fits`` hands to ``read_data_fits`` (spectral_cube/io/
    fits.py:63-172) for an image HDU, as the cube's float32 (or, out_dtype=
    np.float64 for BITPIX -64 / 32 / 64, in the file's own precision):
    big-endian payload -> native; the multiply by BSCALE (when it is not 1) and
    the add of BZERO (when it is not 0) are two roundings, in float32 for
    BITPIX 8/16, float64 for 32/64 and the file's own precision for floating
    types; BITPIX 32/64 reach float32 THROUGH float64 also when unscaled (the
    reference's cube of an integer image is np.result_type(dtype, 0.0),
    masks.py:225); BITPIX 64 with BSCALE 1, BZERO 2**63 is the uint64 the
    file means, rounded once; integer BLANK -> NaN.
    gen_golden pins this against astropy reading real files
    (case_fits_files, case_fits_decode_edges).

    The FITS standard is followed where astropy 4.3.1 leaves it:
    BLANK acts on the raw integer whenever BITPIX > 0 - also ``BLANK = 0``
    (astropy tests ``if self._blank:``) and on the pseudo-unsigned images
    BSCALE 1, BZERO 2**15 / 2**31 / 2**63 (and BZERO -128 of BITPIX 8), where
    astropy hands out an unsigned array and forgets BLANK.
    astropy_quirks=True reproduces astropy on these."""
    dt = {8: ">u1", 16: ">i2", 32: ">i4", 64: ">i8", -32: ">f4", -64: ">f8"}[bitpix]
    out_dtype = np.dtype(out_dtype).type
    if out_dtype is np.float64 and bitpix not in (-64, 32, 64):
        raise ValueError("float64 output is for BITPIX -64 / 32 / 64")
    a = np.frombuffer(raw, dtype=dt, count=int(np.prod(shape))).reshape(shape)
    if bitpix < 0:
        v = a.astype(a.dtype.newbyteorder("="))
        with np.errstate(all="ignore"):                    # (signalling NaNs, float64 beyond float32's range)
            if bscale != 1.0:
                v = v * v.dtype.type(bscale)
            if bzero != 0.0:
                v = v + v.dtype.type(bzero)
            return v.astype(out_dtype)
    pseudo = bscale == 1.0 and bzero == {8: -128.0, 16: 2.0 ** 15, 32: 2.0 ** 31, 64: 2.0 ** 63}[bitpix]
    if astropy_quirks and (pseudo or blank == 0):
        blank = None
    work = np.float32 if bitpix in (8, 16) else np.float64
    if bitpix == 64 and pseudo:
        v = (a.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)).astype(out_dtype)     # one rounding
    else:
        v = a.astype(work)
        if bscale != 1.0:
            v *= work(bscale)
        if bzero != 0.0:
            v += work(bzero)
    if blank is not None:
        v[a == blank] = np.nan
    return v.astype(out_dtype)


# --------------------------------------------------------------------------
# order statistics along an axis
# --------------------------------------------------------------------------
def median(data, include=None, axis=0):
    """``DaskSpectralCubeMixin.median`` (spectral_cube/dask_spectral_cube.py:657-
    671): nanmedian of the NaN-filled data along *axis*; all-NaN rays -> NaN."""
    import warnings
    d = filled(data, include, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmedian(d, axis=axis)


def percentile(data, include, q, axis=0):
    """``percentile`` (dask_spectral_cube.py:673-693): np.nanpercentile (linear
    interpolation between the two bracketing order statistics)."""
    import warnings
    d = filled(data, include, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanpercentile(d, q, axis=axis)


def mad_std(data, include=None, axis=0):
    """``mad_std`` (dask_spectral_cube.py:711-731) = astropy.stats.mad_std(
    ignore_nan=True): 1.482602218505602 * nanmedian(|x - nanmedian(x)|)."""
    import warnings
    d = filled(data, include, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        med = np.nanmedian(d, axis=axis, keepdims=True)
        return 1.482602218505602 * np.nanmedian(np.abs(d - med), axis=axis)


def sigma_clip(data, include=None, sigma=3.0, maxiters=5, cenfunc="median", stdfunc="std",
               sigma_lower=None, sigma_upper=None, out_dtype=np.float32):
    """``astropy.stats.sigma_clip(array, sigma, axis=0, masked=False, copy=True)`` as called by
    ``sigma_clip_spectrally`` (spectral_cube/dask_spectral_cube.py:851-878): iterate
    bounds = centre -/+ sigma*std per ray (nan-aware), values outside -> NaN, until a pass
    clips nothing or *maxiters* passes were made.  float64 internally."""
    import warnings
    lo_s = sigma if sigma_lower is None else sigma_lower
    hi_s = sigma if sigma_upper is None else sigma_upper
    f = filled(data, include, np.nan).astype(np.float64)
    it = 0
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        while maxiters is None or it < maxiters:
            it += 1
            cen = np.nanmedian(f, axis=0) if cenfunc == "median" else np.nanmean(f, axis=0)
            if stdfunc == "std":
                std = np.nanstd(f, axis=0)
            else:
                std = 1.482602218505602 * np.nanmedian(np.abs(f - np.nanmedian(f, axis=0)), axis=0)
            out = (f < cen - lo_s * std) | (f > cen + hi_s * std)
            if not out.any():
                break
            f[out] = np.nan
    return f.astype(out_dtype)


# --------------------------------------------------------------------------
# Gaussian beam algebra behind convolve_to.
# PARITY UNPINNED against radio_beam (third party: pyproject.toml lists `radio_beam`, no pin, absent from this
# image).  The reference calls ``beam.deconvolve(self.beam).as_kernel(pixscale)`` (dask_spectral_cube.py:1445-1447,
# spectral_cube.py:3378-3420); its tests hold one known answer reproducible without the package (a circular 1"
# beam convolved to 1.5": kernel FWHM sqrt(1.5^2 - 1^2), tests/test_regrid.py:32-56).  What follows is an
# INDEPENDENT restatement - second-moment matrices and an eigen-decomposition, not the closed-form of the
# product's beam.py (Wild 1970 via radio_beam.utils.deconvolve) - so that the product is not compared with itself.
# --------------------------------------------------------------------------
_FWHM_TO_SIGMA = 1.0 / np.sqrt(8.0 * np.log(2.0))


def beam_second_moments(major, minor, pa_deg):
    """2 x 2 second-moment matrix (same units as major^2, Gaussian sigma^2) of an elliptical Gaussian beam in
    image axes (x to the right, y up); the position angle runs from +y towards -x (north through east on a sky
    image whose x axis is RA increasing to the left)."""
    u = np.array([-np.sin(np.radians(pa_deg)), np.cos(np.radians(pa_deg))])      # unit vector along the major axis
    v = np.array([u[1], -u[0]])                                                  # and along the minor axis
    sa, sb = major * _FWHM_TO_SIGMA, minor * _FWHM_TO_SIGMA
    return sa * sa * np.outer(u, u) + sb * sb * np.outer(v, v)


def beam_from_second_moments(cov):
    """(major, minor, pa_deg) FWHM of the Gaussian with second-moment matrix *cov*; pa in (-90, 90]"""
    w, vecs = np.linalg.eigh(np.asarray(cov, dtype=np.float64))                   # ascending eigenvalues
    major, minor = np.sqrt(max(w[1], 0.0)) / _FWHM_TO_SIGMA, np.sqrt(max(w[0], 0.0)) / _FWHM_TO_SIGMA
    ux, uy = vecs[0, 1], vecs[1, 1]
    pa = np.degrees(np.arctan2(-ux, uy))
    pa = (pa + 90.0) % 180.0 - 90.0
    if pa == -90.0:
        pa = 90.0
    if abs(w[1] - w[0]) <= 1e-14 * abs(w[1]):
        pa = 0.0                                                                 # circular: no direction
    return major, minor, pa


def deconvolve_beam(target, current, rel_slack=1e-7):
    """(major, minor, pa_deg) of the Gaussian that, convolved with *current*, gives *target* (both
    (major, minor, pa_deg)): second moments subtract under deconvolution.  Raises ValueError when the difference
    is not a valid (positive semi-definite, non-zero) second-moment matrix - the target is smaller than, or
    equal to, the current beam along some direction."""
    diff = beam_second_moments(*target) - beam_second_moments(*current)
    w = np.linalg.eigvalsh(diff)
    scale = min(target[1], current[1]) ** 2 * _FWHM_TO_SIGMA ** 2
    if w[0] < -rel_slack * scale or w[1] <= rel_slack * scale:
        raise ValueError("beam could not be deconvolved")
    return beam_from_second_moments(diff)


def elliptical_gaussian_kernel(major, minor, pa_deg, pixscale, support_scaling=8.0):
    """Sampled (pixel centres, NOT normalised to unit sum: amplitude 1 / (2 pi sx sy)) elliptical Gaussian of FWHM
    major x minor and position angle pa on a grid of *pixscale* per pixel: support = 8 x the larger sigma rounded
    up to an odd number of pixels (the published sizing of radio_beam's EllipticalGaussian2DKernel)."""
    sx, sy = major * _FWHM_TO_SIGMA / pixscale, minor * _FWHM_TO_SIGMA / pixscale
    size = int(np.ceil(support_scaling * max(sx, sy)))
    size += 1 - size % 2
    h = size // 2
    yy, xx = np.mgrid[-h:h + 1, -h:h + 1].astype(np.float64)
    t = np.radians(pa_deg)
    along = -np.sin(t) * xx + np.cos(t) * yy                                     # coordinate along the major axis
    across = np.cos(t) * xx + np.sin(t) * yy
    return np.exp(-0.5 * ((along / sx) ** 2 + (across / sy) ** 2)) / (2.0 * np.pi * sx * sy)
