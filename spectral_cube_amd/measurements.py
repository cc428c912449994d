"""Per-label measurements of a cube on the device: the scipy.ndimage measurement family over a LabelMap, and a catalogue.

What users of the reference do on the host with ``scipy.ndimage.sum_labels``, ``mean``, ``variance``, ``minimum_position``,
``center_of_mass`` ... on the label array and ``cube.filled_data[:]``, here where both live: one streaming segmented
reduction of the cube through its labels (ops.label_measure, csrc/spc_label_measure.hip), after which only tables of
n + 1 rows travel to the host.  The functions carry scipy's names, take ``(cube, labels, index=None)`` with *labels* a
:class:`~spectral_cube_amd.labelling.LabelMap`, and return what their namesakes return.

A voxel is measured when its label is above 0, the cube's mask includes it and its sample is not NaN: the results equal
scipy run on ``np.where(include, data, 0)`` with the labels ``np.where(include & ~isnan(data), labels, 0)``.  *index*: a
label number gives a scalar (a tuple for a position), a sequence of numbers in 1 ... n gives arrays (lists of tuples),
duplicates allowed; None measures all labelled voxels as one region.  0 or a number above n raises ValueError: the
background is not measured.  A label without a measured voxel gives sum 0, NaN for mean, variance and extrema and the
position (-1, -1, -1) (scipy's 0.0 and (0, 0, 0) there are artefacts of its implementation).

The arithmetic after the kernel - means, variances, centroids, dispersions, *index* and the union of None - is in the
``*_from`` functions below: pure numpy on the raw tables, no device.  Every sum of the tables is float64; variances are
two-pass (the second call measures about the means of the first), scipy's own form.  scipy itself is never imported.
"""
import numpy as np

from . import ops

__all__ = ["sum_labels", "mean", "variance", "standard_deviation", "minimum", "maximum", "minimum_position",
           "maximum_position", "extrema", "center_of_mass"]


# ---- pure numpy on the raw tables ---------------------------------------------------------------------------------------
def parse_index(index, n):
    """(label numbers int64 (m,), scalar) of *index* for labels 1 ... *n*; (None, True) for None, the union"""
    if index is None:
        return None, True
    idx = np.asarray(index)
    if idx.dtype == bool or idx.dtype.kind not in "iuf" or idx.ndim > 1:
        raise ValueError("index must be a label number or a sequence of label numbers (got %r)" % (index,))
    if idx.dtype.kind == "f":
        if idx.size and not np.array_equal(idx, np.floor(idx)):
            raise ValueError("label numbers must be whole numbers (got %r)" % (index,))
    num = idx.astype(np.int64).ravel()
    if num.size and (num.min() < 1 or num.max() > n):
        raise ValueError("label numbers must be 1 to %d: the background (0) is not measured (got %r)" % (n, index))
    return num, idx.ndim == 0


def _pick(values, sel, scalar):
    """the rows *sel* of a per-label array, as a scalar for a scalar index"""
    out = np.asarray(values)[sel]
    return out[0] if scalar else out


def _coords(pos, shape):
    """(m, 3) int64 z, y, x of linear C-order positions; -1 stays (-1, -1, -1)"""
    pos = np.asarray(pos, np.int64)
    ok = pos >= 0
    z, y, x = np.unravel_index(np.where(ok, pos, 0), shape)
    return np.where(ok[:, None], np.stack([z, y, x], axis=1), -1).astype(np.int64)


def _tuples(rows, scalar):
    """scipy's form of positions: a tuple for a scalar index, a list of tuples for a sequence"""
    out = [tuple(r.tolist()) for r in np.asarray(rows)]
    return out[0] if scalar else out


def sum_from(t, index, n):
    """sum_labels from the tables of a pass about v0 = 0 (``count``, ``sums``)"""
    sel, scalar = parse_index(index, n)
    total = np.asarray(t["sums"], np.float64)[:, 0]
    if sel is None:
        return total[1:].sum()
    return _pick(total, sel, scalar)


def mean_from(t, index, n):
    """mean from the tables of a pass about v0 = 0; NaN for a label with nothing measured"""
    sel, scalar = parse_index(index, n)
    count, total = np.asarray(t["count"], np.int64), np.asarray(t["sums"], np.float64)[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        if sel is None:
            c = count[1:].sum()
            return total[1:].sum() / c if c else np.float64(np.nan)
        return _pick(np.where(count > 0, total / np.where(count > 0, count, 1), np.nan), sel, scalar)


def variance_origin(t, index, n):
    """(n + 1, 4) origin table of the second pass of a variance: v0 = every label's mean, or (index None) the mean of
    the union for all of them; 0 where nothing is measured"""
    count, total = np.asarray(t["count"], np.int64), np.asarray(t["sums"], np.float64)[:, 0]
    origin = np.zeros((n + 1, 4), np.float64)
    if index is None:
        c = count[1:].sum()
        origin[1:, 0] = total[1:].sum() / c if c else 0.0
    else:
        origin[:, 0] = np.where(count > 0, total / np.where(count > 0, count, 1), 0.0)
        origin[0, 0] = 0.0
    return origin


def variance_from(t2, index, n):
    """variance from the tables of the pass about the means (variance_origin): sum (v - mean)^2 / count, scipy's form"""
    sel, scalar = parse_index(index, n)
    count, sq = np.asarray(t2["count"], np.int64), np.asarray(t2["sums"], np.float64)[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        if sel is None:
            c = count[1:].sum()
            return sq[1:].sum() / c if c else np.float64(np.nan)
        return _pick(np.where(count > 0, sq / np.where(count > 0, count, 1), np.nan), sel, scalar)


def _union_extreme(values, pos, largest):
    """(value, position) of the extreme over all labels: NaN rows (nothing measured) are passed over, the smallest
    position wins a tie"""
    values, pos = np.asarray(values)[1:], np.asarray(pos, np.int64)[1:]
    ok = pos >= 0
    if not ok.any():
        return values.dtype.type(np.nan), np.int64(-1)
    v = values[ok].max() if largest else values[ok].min()
    return v, pos[ok & (values == v)].min()


def extreme_from(t, index, n, largest):
    """minimum (*largest* False) or maximum: the cube's dtype, NaN for a label with nothing measured"""
    sel, scalar = parse_index(index, n)
    key = "max" if largest else "min"
    if sel is None:
        return _union_extreme(t[key], t[key + "_pos"], largest)[0]
    return _pick(t[key], sel, scalar)


def position_from(t, index, n, shape, largest):
    """minimum_position / maximum_position: (z, y, x) of the first extreme in C order, (-1, -1, -1) without one"""
    sel, scalar = parse_index(index, n)
    key = "max_pos" if largest else "min_pos"
    if sel is None:
        return _tuples(_coords([_union_extreme(t[key[:3]], t[key], largest)[1]], shape), True)
    return _tuples(_coords(np.asarray(t[key])[sel], shape), scalar)


def extrema_from(t, index, n, shape):
    """(minimums, maximums, min_positions, max_positions), scipy.ndimage.extrema"""
    return (extreme_from(t, index, n, False), extreme_from(t, index, n, True),
            position_from(t, index, n, shape, False), position_from(t, index, n, shape, True))


def centroid_table(first, origin=None):
    """(n + 1, 3) float64: the intensity-weighted centroid z, y, x of every label from the ``first`` table of a pass about
    *origin* ((n + 1, 4), None: zero) - origin + sum v (coord - origin) / sum v; NaN where sum v is 0 or nothing is measured"""
    first = np.asarray(first, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = first[:, 1:4] / first[:, :1]
    return c if origin is None else c + np.asarray(origin, np.float64)[:, 1:4]


def center_of_mass_from(t, index, n):
    """center_of_mass from the ``first`` table of a pass about the zero origin: sum v coord / sum v"""
    sel, scalar = parse_index(index, n)
    first = np.asarray(t["first"], np.float64)
    if sel is None:
        s = first[1:].sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return tuple((s[1:4] / s[0]).tolist())
    return _tuples(centroid_table(first)[sel], scalar)


def box_origin(sizes, bbox):
    """(n + 1, 4) origin table of the catalogue's first pass: v0 = 0 and the low corner of every label's bounding box
    (LabelMap.bounding_boxes), so the coordinates a label sums stay small; zero for a label without a voxel"""
    bbox = np.asarray(bbox).reshape(-1, 6)
    origin = np.zeros((bbox.shape[0], 4), np.float64)
    origin[:, 1:] = np.where(np.asarray(sizes)[:, None] > 0, bbox[:, 0::2], 0)
    origin[0] = 0.0
    return origin


def catalog_from(t1, origin1, t2, centroid, shape, channel_width=1.0, wcs=None):
    """The catalogue from the raw tables of its two passes, pure numpy: *t1* (count, sums, min .. max_pos, first) measured
    about *origin1* (box_origin), *t2* (second) about *centroid* = centroid_table(t1["first"], origin1).  A dict of arrays
    of length n, label k in row k - 1:

    npix (int64), flux = sum v * |channel_width|, peak, peak_position (n, 3), centroid (n, 3: z, y, x in pixels),
    sigma_z / sigma_y / sigma_x = sqrt(sum v d^2 / sum v) about the centroid, position_angle = half the angle
    atan2(2 mu_yx, mu_xx - mu_yy) of the (y, x) moment ellipse's major axis, in radians from +x towards +y.  With *wcs*
    (a linear spectral axis): v_cen = the axis at the z centroid, sigma_v = sigma_z |channel width|, and, where the WCS
    has a celestial part, lon / lat of the centroid in degrees (SimpleWCS.celestial_pix2world)."""
    first, second = np.asarray(t1["first"], np.float64), np.asarray(t2["second"], np.float64)
    w = first[1:, 0]
    cen = np.asarray(centroid, np.float64)[1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = second[1:] / w[:, None]                   # zz, yy, xx, zy, zx, yx
        sig = np.sqrt(mu[:, :3])
        pa = 0.5 * np.arctan2(2.0 * mu[:, 5], mu[:, 2] - mu[:, 1])
    pa = np.where(np.isfinite(mu[:, [1, 2, 5]]).all(axis=1), pa, np.nan)
    cat = {"npix": np.asarray(t1["count"], np.int64)[1:].copy(),
           "flux": np.asarray(t1["sums"], np.float64)[1:, 0] * abs(float(channel_width)),
           "peak": np.asarray(t1["max"])[1:].copy(),
           "peak_position": _coords(np.asarray(t1["max_pos"])[1:], shape),
           "centroid": cen, "sigma_z": sig[:, 0], "sigma_y": sig[:, 1], "sigma_x": sig[:, 2], "position_angle": pa}
    if wcs is not None:
        cat["v_cen"] = np.asarray(wcs.spectral_pix2world(cen[:, 0]), np.float64)
        cat["sigma_v"] = sig[:, 0] * abs(float(channel_width))
        ok = np.isfinite(cen).all(axis=1)
        try:
            lon, lat = wcs.celestial_pix2world(np.where(ok, cen[:, 2], 0.0), np.where(ok, cen[:, 1], 0.0))
        except (AttributeError, ValueError, NotImplementedError):       # a spectral-only WCS, a projection that is not built
            pass
        else:
            cat["lon"], cat["lat"] = np.where(ok, lon, np.nan), np.where(ok, lat, np.nan)
    return cat


# ---- the device passes --------------------------------------------------------------------------------------------------
def measure(cube, labels, want=("sums", "extrema", "first"), origin=None):
    """{table: host array of n + 1 rows}: one ops.label_measure pass of *cube* through the LabelMap *labels* (the raw
    tables the functions of this module derive from; row 0, the background, is never measured)"""
    if tuple(labels.shape) != tuple(cube.shape):
        raise ValueError("the labels %s and the cube %s must have one shape" % (tuple(labels.shape), tuple(cube.shape)))
    if cube._stream_source() is not None:
        raise NotImplementedError("measuring labels needs the whole cube in HBM: an out-of-core cube is refused "
                                  "(as labelling refuses it)")
    data, spec, _ = cube._operand()
    tables = ops.label_measure(data, labels.device_array(), labels.n, mask_spec=spec, origin=origin, want=want)
    return {k: v.get() for k, v in tables.items()}


def sum_labels(cube, labels, index=None):
    """scipy.ndimage.sum_labels: the sum of the measured samples of every label of *index*"""
    parse_index(index, labels.n)
    return sum_from(measure(cube, labels, ("sums",)), index, labels.n)


def mean(cube, labels, index=None):
    """scipy.ndimage.mean"""
    parse_index(index, labels.n)
    return mean_from(measure(cube, labels, ("sums",)), index, labels.n)


def variance(cube, labels, index=None):
    """scipy.ndimage.variance, two-pass: the second pass sums (v - mean)^2 about the means of the first"""
    parse_index(index, labels.n)
    origin = variance_origin(measure(cube, labels, ("sums",)), index, labels.n)
    return variance_from(measure(cube, labels, ("sums",), origin=origin), index, labels.n)


def standard_deviation(cube, labels, index=None):
    """scipy.ndimage.standard_deviation: the square root of :func:`variance`"""
    return np.sqrt(variance(cube, labels, index))


def minimum(cube, labels, index=None):
    """scipy.ndimage.minimum"""
    parse_index(index, labels.n)
    return extreme_from(measure(cube, labels, ("extrema",)), index, labels.n, False)


def maximum(cube, labels, index=None):
    """scipy.ndimage.maximum"""
    parse_index(index, labels.n)
    return extreme_from(measure(cube, labels, ("extrema",)), index, labels.n, True)


def minimum_position(cube, labels, index=None):
    """scipy.ndimage.minimum_position: (z, y, x) of the first minimum in C order"""
    parse_index(index, labels.n)
    return position_from(measure(cube, labels, ("extrema",)), index, labels.n, labels.shape, False)


def maximum_position(cube, labels, index=None):
    """scipy.ndimage.maximum_position"""
    parse_index(index, labels.n)
    return position_from(measure(cube, labels, ("extrema",)), index, labels.n, labels.shape, True)


def extrema(cube, labels, index=None):
    """scipy.ndimage.extrema: (minimums, maximums, min_positions, max_positions) from one pass"""
    parse_index(index, labels.n)
    return extrema_from(measure(cube, labels, ("extrema",)), index, labels.n, labels.shape)


def center_of_mass(cube, labels, index=None):
    """scipy.ndimage.center_of_mass: sum v coord / sum v, (z, y, x) in pixels"""
    parse_index(index, labels.n)
    return center_of_mass_from(measure(cube, labels, ("first",)), index, labels.n)


def catalog(cube, labels):
    """The cloud catalogue of :func:`catalog_from` in two passes: sums, extrema and first moments about every label's
    box corner, then the second moments about the centroids (the reference's two-pass moment 2, _moments.py:185-193, per
    region instead of per spaxel).  ``flux_unit`` and the units of the WCS columns are in ``cat["meta"]``."""
    n = labels.n
    origin1 = box_origin(labels.sizes(), labels.bounding_boxes())
    t1 = measure(cube, labels, ("sums", "extrema", "first"), origin=origin1)
    centroid = centroid_table(t1["first"], origin1)
    origin2 = np.zeros((n + 1, 4), np.float64)
    origin2[:, 1:] = np.where(np.isfinite(centroid), centroid, 0.0)
    t2 = measure(cube, labels, ("second",), origin=origin2)
    wcs = cube.wcs if cube.wcs is not None and hasattr(cube.wcs, "spectral_pix2world") else None
    width = 1.0
    if wcs is not None:
        width = float(wcs.spectral_pix2world(1.0) - wcs.spectral_pix2world(0.0))
    # (the second moments are about origin2: where the centroid is not finite they are NaN through the division by sum v)
    cat = catalog_from(t1, origin1, t2, centroid, labels.shape, channel_width=width, wcs=wcs)
    unit, sunit = str(cube.unit or ""), str(cube.spectral_unit or "")
    cat["meta"] = {"flux_unit": ("%s %s" % (unit, sunit)).strip() if wcs is not None else unit,
                   "spectral_unit": sunit, "channel_width": width, "n": n}
    return cat
