"""combine_headers and mosaic_cubes of spectral_cube.cube_utils (cube_utils.py:751-856): several overlapping fields put
on one sky grid and averaged where they overlap.

``combine_headers`` restates ``reproject.mosaicking.find_optimal_celestial_wcs`` (which the reference calls with
``auto_rotate=False``) on this package's WCS.  ``mosaic_cubes`` runs as ONE kernel (``ops.mosaic``) after one device pixel
map per cube when every cube is resident, of one sample type, on the channels of the first and the order is nearest or
bilinear; everything else goes through ``SpectralCube.reproject`` cube by cube and is added up in float64 on the host.
"""
import re
import warnings

import numpy as np

from . import _lib, masks as M, ops
from .wcs import (SimpleWCS, parse_header, frame_transform, apply_frame_transform, check_same_spectral_kind,
                  spectral_unit_scale, _PROJ_CODE, _SIP_COEF, _SIP_META, _PV_KEY)

_D2R = np.pi / 180.0
_MATRIX_KEY = re.compile(r"^(?:PC|CD)(\d)_(\d)$|^PC00(\d)00(\d)$|^CROTA(\d)$")
_ORDERS = {"nearest-neighbor": 0, "bilinear": 1, "biquadratic": 2, "bicubic": 3}
_IGNORED_KWARGS = ("use_memmap", "roundtrip_coords", "block_size")


def _unit_vectors(lon, lat):
    lo, la = np.asarray(lon, dtype=np.float64) * _D2R, np.asarray(lat, dtype=np.float64) * _D2R
    return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])


def _lonlat(v):
    return np.mod(np.arctan2(v[1], v[0]) / _D2R, 360.0), np.arctan2(v[2], np.hypot(v[0], v[1])) / _D2R


def _celestial_input(header):
    """(SimpleWCS of the two sky axes, (ny, nx)) of a cube or image header"""
    h = parse_header(header)
    w = SimpleWCS(h, naxis=2)
    w._require_celestial()
    if "NAXIS1" not in h or "NAXIS2" not in h:
        raise ValueError("combine_headers needs NAXIS1 and NAXIS2 in both headers (the shapes of the fields)")
    return w, (int(h["NAXIS2"]), int(h["NAXIS1"]))


def _frame_ctypes(frame):
    if frame[0] == "galactic":
        return "GLON", "GLAT"
    if frame[0] in ("icrs", "fk5", "fk4", "fk4-no-e"):
        return "RA--", "DEC-"
    raise NotImplementedError("celestial frame %r of the first header is not built for combine_headers" % (frame,))


def combine_headers(header1, header2, **kwargs):
    """A header (a dict) of the smallest unrotated field that holds both input fields (cube_utils.py:751-789 ->
    ``reproject.mosaicking.find_optimal_celestial_wcs([(shape1, wcs1), (shape2, wcs2)], auto_rotate=False, **kwargs)``).

    The steps: the frame is the first header's; every input gives its four outer corners (0-based pixels (-0.5, -0.5) ...
    (nx - 0.5, ny - 0.5)) and the sky position of its CRPIX; the reference position is the normalised mean of the CRPIX
    positions as unit vectors (``reference=(lon, lat)`` in degrees overrides it); the resolution is the smallest
    ``proj_plane_pixel_scales`` value of the inputs (``resolution=`` in degrees overrides it); the target is
    ``projection`` ('TAN' by default, any code SimpleWCS builds) with CDELT = (-res, +res), no rotation and default
    LONPOLE / LATPOLE; CRPIX puts the smallest projected corner coordinate of each axis on the outer edge of the first
    pixel and NAXISn = round(max - min).  The result is a copy of *header1* with NAXIS = 3, NAXIS3 of *header1*,
    WCSAXES = 3 and the celestial keywords overwritten.

    Divergence: the target is unrotated by definition, so the copy drops ``PCi_j`` / ``CDi_j`` / ``CROTAn`` (a spectral
    scale they carried goes to CDELT3), the SIP and PV cards and LONPOLE / LATPOLE of *header1*; the reference leaves them
    stale.  ``frame=`` and any other keyword raise NotImplementedError; ``auto_rotate`` raises TypeError (the reference
    passes it itself)."""
    if "auto_rotate" in kwargs:
        raise TypeError("find_optimal_celestial_wcs() got multiple values for keyword argument 'auto_rotate'")
    projection = kwargs.pop("projection", "TAN")
    resolution = kwargs.pop("resolution", None)
    reference = kwargs.pop("reference", None)
    for k in kwargs:
        raise NotImplementedError("combine_headers keyword %r is not built (built: projection, resolution, reference)" % k)
    projection = str(projection).upper()
    if projection not in _PROJ_CODE:
        raise NotImplementedError("projection %r not supported by SimpleWCS (built: %s)" % (projection, ", ".join(sorted(_PROJ_CODE))))
    h1 = parse_header(header1)
    inputs = [_celestial_input(h1), _celestial_input(header2)]
    frame = inputs[0][0].frame
    lon_name, lat_name = _frame_ctypes(frame)
    corners, refs, scales = [], [], []
    for w, (ny, nx) in inputs:
        xc = np.array([-0.5, nx - 0.5, nx - 0.5, -0.5])
        yc = np.array([-0.5, -0.5, ny - 0.5, ny - 0.5])
        lon, lat = w.celestial_pix2world(np.append(xc, w.crpix[0] - 1.0), np.append(yc, w.crpix[1] - 1.0))
        v = _unit_vectors(lon, lat)
        tr = frame_transform(w.frame, frame)                  # NotImplementedError for pairs that are not built
        if tr is not None:
            v = apply_frame_transform(tr, v)
        corners.append(v[:, :4])
        refs.append(v[:, 4])
        scales.append(np.sqrt((w._lin2() ** 2).sum(axis=0)))   # astropy.wcs.utils.proj_plane_pixel_scales
    if reference is None:
        mean = np.mean(np.stack(refs), axis=0)
        ref_lon, ref_lat = _lonlat(mean / np.sqrt((mean ** 2).sum()))
    else:
        ref_lon, ref_lat = (float(x) for x in reference)
    if resolution is None:
        resolution = float(np.min(np.stack(scales)))
    elif hasattr(resolution, "to"):
        resolution = float(resolution.to("deg").value)
    else:
        resolution = float(resolution)
    celestial = {"CTYPE1": "%-4s-%s" % (lon_name, projection), "CTYPE2": "%-4s-%s" % (lat_name, projection),
                 "CUNIT1": "deg", "CUNIT2": "deg", "CRVAL1": float(ref_lon), "CRVAL2": float(ref_lat),
                 "CDELT1": -resolution, "CDELT2": resolution, "CRPIX1": 1.0, "CRPIX2": 1.0}
    for k in ("RADESYS", "RADECSYS", "EQUINOX", "EPOCH"):
        if k in h1:
            celestial[k] = h1[k]
    target = SimpleWCS(celestial, naxis=2)
    xp, yp = target.celestial_world2pix(*_lonlat(np.concatenate(corners, axis=1)))
    if not (np.all(np.isfinite(xp)) and np.all(np.isfinite(yp))):
        raise ValueError("a corner of an input field cannot be projected onto the %s grid at (%.6f, %.6f)"
                         % (projection, ref_lon, ref_lat))
    xmin, xmax, ymin, ymax = xp.min(), xp.max(), yp.min(), yp.max()
    celestial["CRPIX1"], celestial["CRPIX2"] = float(0.5 - xmin), float(0.5 - ymin)
    naxis1, naxis2 = int(round(xmax - xmin)), int(round(ymax - ymin))

    w1 = SimpleWCS(h1, strict=False)
    out = {}
    for k, v in h1.items():
        if _MATRIX_KEY.match(k) or _SIP_COEF.match(k) or _SIP_META.match(k) or k in ("LONPOLE", "LATPOLE"):
            continue
        m = _PV_KEY.match(k)
        if m and int(m.group(2)) <= 2:
            continue
        out[k] = v
    if w1.naxis >= 3:
        if np.any(w1.pc[2, :2] != 0.0) or np.any(w1.pc[:2, 2] != 0.0):
            raise NotImplementedError("combine_headers: the first header couples the spectral axis to the sky axes (PCi_3 / PC3_j)")
        if any(_MATRIX_KEY.match(k) for k in h1):
            out["CDELT3"] = float(w1.cdelt[2] * w1.pc[2, 2])
    out["NAXIS"] = 3
    out["NAXIS1"], out["NAXIS2"] = naxis1, naxis2
    out["NAXIS3"] = h1["NAXIS3"]
    out.update(celestial)
    out["WCSAXES"] = 3
    return out


def _cube_header(cube):
    """the cube's header with NAXISn of its shape (the reference's ``cube.header`` always carries them)"""
    h = dict(cube.header)
    h["NAXIS"] = 3
    h["NAXIS3"], h["NAXIS2"], h["NAXIS1"] = (int(n) for n in cube.shape)
    return h


def _same_channels(cube, newwcs):
    """True when *newwcs* asks for the channels *cube* has: the test ``SpectralCube.reproject`` makes before it decides on
    a purely spatial reprojection"""
    nz = cube.shape[0]
    if not (newwcs.naxis >= 3 and cube._wcs is not None and cube._wcs.naxis >= 3):
        return True
    nz_out = int(newwcs.header.get("NAXIS3", nz))
    check_same_spectral_kind(cube._wcs, newwcs)
    scale = spectral_unit_scale(newwcs.spectral_unit or cube.spectral_unit, cube.spectral_unit)
    zs = cube._wcs.spectral_world2pix(newwcs.spectral_pix2world(np.arange(nz_out)) * scale)
    return nz_out == nz and bool(np.all(np.abs(zs - np.arange(nz)) <= 1e-9 * max(nz, 1)))


def mosaic_route(cubes, newwcs, order):
    """'fused' (one kernel) or 'composed' (reproject per cube, float64 sums on the host) for these inputs"""
    if order not in (0, 1):
        return "composed"
    wide = [bool(c._runs_wide()) for c in cubes]
    if any(w != wide[0] for w in wide):
        return "composed"
    try:
        return "fused" if all(_same_channels(c, newwcs) for c in cubes) else "composed"
    except NotImplementedError:             # (another spectral representation: reproject refuses it in its own words)
        return "composed"


def _fused(cubes, newwcs, shape_yx, order, filled):
    wide = bool(cubes[0]._runs_wide())
    datas, maps, masks, fills = [], [], [], []
    for c in cubes:
        c._wcs._require_celestial()
        data = c._device_data64() if wide else c._device_data()
        mask = (c._mask_spec64() if wide else c._mask_spec()) if filled else None
        fill = float(c._fill_value)
        if filled and not np.isnan(fill) and c._mask is not None and M.contains(c._mask, M.NotNaNMask) \
                and not M.contains(c._mask, M.InvertedMask):
            # ~isnan(data) lowers to nothing, but here the excluded voxels become a fill value that is a number: the NaN
            # samples must be named (as SpectralCube.reproject does)
            mask = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, ops.mask_include(data, mask, nan_excluded=True))
        datas.append(data)
        masks.append(mask)
        fills.append(fill)
        maps.append(ops.wcs_pixel_map(c._wcs, newwcs, shape_yx, c.device))
    return ops.mosaic(datas, maps, masks, fills, order)


def _composed(cubes, newwcs, shape, order, filled):
    final = np.zeros(shape, dtype=np.float64)
    weight = np.zeros(shape[1:], dtype=np.float64)
    for c in cubes:
        r = c.reproject(newwcs, order=order, filled=filled)
        weight += r.get_mask_array()[0].astype(np.float64)          # 2-D: the footprint of channel 0 only
        final += np.nan_to_num(np.asarray(r.filled_data, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        final /= weight
    return final


def mosaic_cubes(cubes, spectral_block_size=100, combine_header_kwargs={}, **kwargs):
    """Reproject *cubes* onto one common sky grid and average them where they overlap (cube_utils.py:791-856).

    The grid is ``combine_headers`` applied pairwise in list order (*combine_header_kwargs* go there) with the first
    cube's spectral axis.  Per cube, in list order: ``reproject`` onto it (``order`` and ``filled`` are passed on; masked
    voxels enter as the cube's fill value), ``weight += footprint`` and ``final += nan_to_num(filled data)`` in float64;
    then ``final /= weight``.  Three things follow, as in the reference: a NaN inside a footprint counts as a zero with
    weight 1; the weight is a 2-D map - where a cube's footprint varies with channel (its channels differ from the first
    cube's), channel 0 decides; a cube whose fill value is a number contributes it outside its footprint too.  No cube
    reaches a pixel: NaN.

    One kernel after one device pixel map per cube (no reprojected cube is written) when the order is nearest or bilinear,
    every cube is resident, all are float32 or all float64, and every cube has the first cube's channels; spline orders,
    other spectral axes and mixed sample types reproject cube by cube and add up in float64 on the host (there, as in
    ``reproject``, a cube that misses the grid raises ValueError).  An out-of-core cube raises HugeCubeError.

    The result is resident on the device: a plain SpectralCube (also for a first cube with beams) of the first cube's
    unit, ``wcs=SimpleWCS(header)``, a finite-value mask, no beam and no meta.  Cubes of different units give a UserWarning
    and the first unit wins (the reference ignores units silently).  Divergence: the reference returns float64 whatever went
    in; here the sums are float64 and the result is rounded ONCE to the cubes' sample type (the first cube's for a mix), as
    ``stack_cube`` does.  ``spectral_block_size``, ``use_memmap``, ``roundtrip_coords`` and ``block_size`` are accepted and
    ignored; any other keyword is a TypeError."""
    from . import streaming
    from .cube import SpectralCube
    from .device import DeviceArray
    cubes = list(cubes)
    if not cubes:
        raise ValueError("an empty list of cubes")
    order = kwargs.pop("order", "bilinear")
    filled = kwargs.pop("filled", True)
    for k in _IGNORED_KWARGS:
        kwargs.pop(k, None)
    for k in kwargs:
        raise TypeError("mosaic_cubes() got an unexpected keyword argument %r" % k)
    order_n = _ORDERS.get(order, order)
    if order_n not in (0, 1, 2, 3):
        raise ValueError("order %r: 'nearest-neighbor' (0), 'bilinear' (1), 'biquadratic' (2) or 'bicubic' (3)" % (order,))
    first = cubes[0]
    header = _cube_header(first)
    for cu in cubes[1:]:
        header = combine_headers(header, _cube_header(cu), **dict(combine_header_kwargs))
    units = [str(c.unit or "") for c in cubes]
    if any(u != units[0] for u in units):
        warnings.warn("mosaic_cubes: the cubes have different units (%s); the result carries the first"
                      % ", ".join(sorted(set(units))), UserWarning, stacklevel=2)
    for c in cubes:
        if c._is_huge and not c.allow_huge_operations:       # (reproject is one of the operations the reference guards: utils.py:41-75)
            raise ValueError("mosaic_cubes reprojects every cube, which requires loading the entire cube into memory, and the cube is "
                             "large ({0} pixels), so by default we disable this operation. To enable the operation, set "
                             "`cube.allow_huge_operations=True` and try again.".format(c.size))
        if c._stream_source() is not None:
            raise streaming.HugeCubeError("mosaic_cubes needs every cube resident in HBM: %s is larger than the budget "
                                          "(SPC_HBM_BUDGET) and strip streaming is not built for mosaic_cubes" % (c.shape,))
    newwcs = SimpleWCS(header)
    shape = (int(header["NAXIS3"]), int(header["NAXIS2"]), int(header["NAXIS1"]))
    route = mosaic_route(cubes, newwcs, order_n)
    _lib.require_gpu()
    wide = bool(first._runs_wide())
    if route == "fused":
        dev = _fused(cubes, newwcs, shape[1:], order_n, bool(filled))
    else:
        final = _composed(cubes, newwcs, shape, order_n, bool(filled))
        dev = DeviceArray.from_numpy(np.ascontiguousarray(final, dtype=np.float64 if wide else np.float32), first.device)
    if wide:
        out = first._new_wide_cube(lambda: dev, shape=shape, wcs=newwcs, mask=False, plain=True)
        out._meta, out._fill_value = {}, np.nan
    else:
        out = SpectralCube._new_cube_with(first, dev=dev, wcs=newwcs, mask=False, meta={}, fill_value=np.nan, shape=shape)
    out._mask = M.LazyMask(np.isfinite, cube=out)
    return out
