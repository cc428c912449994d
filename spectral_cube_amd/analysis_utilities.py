"""``stack_spectra`` and ``stack_cube`` of spectral_cube.analysis_utilities.

``stack_spectra`` of spectral_cube.analysis_utilities (analysis_utilities.py:134-318) on the device: every spectrum is
Fourier-shifted by its own number of channels so that the lines align, and the shifted spectra are combined into one.

The host restates the reference's bookkeeping (validation, default positions and ``v0``, the linearity check, the range
masking, the pixel shifts, the padding and the new ``CRPIX1`` / ``NAXIS1``) in its order; every voxel is touched only by
the HIP kernels of spc_stack.hip.  ``np.nanmean`` / ``np.mean`` / ``np.nansum`` / ``np.sum`` never write a shifted spectrum
(``ops.stack_sum``); any other ``stack_function`` receives the ``(P, M)`` array of shifted spectra (``ops.stack_shift``)
on the host, as in the reference.  There is no CPU fallback.

``stack_cube`` (analysis_utilities.py:321-432) stacks the spectral lines of one wide-band frequency cube on the velocity
grid of the first: the host plans the slabs and the interpolation tables (``stack_cube_plan``), one kernel of
spc_stack_cube.hip reads every slab once and writes the stacked cube (``ops.stack_cube``).
"""
import warnings

import numpy as np

from . import _lib, ops
from .cube import Projection, SmoothingWarning, SpectralCube, UnitsError, _nan_term_dropped
from .wcs import SpectralAxisWCS, _SPECTRAL_SI, spectral_unit_scale


class BadVelocitiesWarning(UserWarning):
    """velocities of the surface lie outside the spectral axis and are masked out (utils.py, BadVelocitiesWarning)"""


# stack functions finished from (sum, count, NaN count) per channel, recognised by identity or by name
_FUSED = ("nanmean", "mean", "nansum", "sum")


def _fused_name(stack_function):
    for name in _FUSED:
        if stack_function is getattr(np, name):
            return name
    name = getattr(stack_function, "__name__", None)
    return name if name in _FUSED else None


def _in_spectral_unit(cube, value):
    """*value* (array or number) in the cube's spectral unit, float64: plain numbers are taken to be in it, anything with
    ``.value`` and ``.unit`` is converted with the rules (and errors) of ``SpectralCube._spectral_value``"""
    if not hasattr(value, "unit"):
        return np.asarray(value, dtype=np.float64)

    class _One:
        pass
    one = _One()
    one.value, one.unit = 1.0, value.unit
    return np.asarray(value.value, dtype=np.float64) * cube._spectral_value(one)


def stack_plan(cube, velocity_surface, v0=None, xy_posns=None, pad_edges=True, vdiff_tol=0.01):
    """the host side of ``stack_spectra`` up to the kernels: (flat spaxel indices, pixel shifts, (pad_lo, pad_hi)), with
    the reference's checks, warnings and arithmetic in its order (analysis_utilities.py:184-275)"""
    vel = _in_spectral_unit(cube, velocity_surface)
    if not np.isfinite(vel).any():
        raise ValueError("velocity_surface contains no finite values.")
    nz, ny, nx = cube.shape
    if tuple(vel.shape) != (ny, nx):
        raise ValueError("Velocity surface map does not match cube spatial dimensions.")
    if xy_posns is None:
        xy_posns = np.where(np.isfinite(vel))          # (before the range masking: an out-of-range velocity stays, as NaN)
    else:
        xy_posns = tuple(xy_posns)
    axis = np.asarray(cube.spectral_axis, dtype=np.float64)
    if v0 is None:
        v0 = axis.mean()
    else:
        v0 = float(cube._spectral_value(v0))
        if v0 < axis.min() or v0 > axis.max():
            raise ValueError("v0 must be within the range of the spectral axis of the cube.")
    if nz < 2:
        raise ValueError("Cannot shift spectra on an axis of one channel")
    spec_size = axis[1] - axis[0]
    sign = -1.0 if spec_size > 0.0 else 1.0            # increasing axis: -1, decreasing: +1
    vdiff = abs(spec_size)
    vdiff2 = abs(axis[-1] - axis[-2])
    if not np.isclose(vdiff2, vdiff, rtol=vdiff_tol):
        raise ValueError("Cannot shift spectra on a non-linear axes")
    vmax, vmin = axis.max(), axis.min()
    with np.errstate(invalid="ignore"):
        if np.any(vel > vmax) or np.any(vel < vmin):
            warnings.warn("Some velocities are outside the allowed range and will be masked out.", BadVelocitiesWarning, stacklevel=3)
            vel = np.where((vel < vmax) & (vel > vmin), vel, np.nan)
    pix_shifts = np.atleast_1d(sign * ((vel - v0) / vdiff)[xy_posns]).astype(np.float64).ravel()
    idx = np.atleast_1d(np.arange(ny * nx, dtype=np.int64).reshape(ny, nx)[xy_posns]).ravel()
    if idx.size == 0:
        raise ValueError("xy_posns names no position")
    pad = (0, 0)
    if pad_edges:
        if not np.isfinite(pix_shifts).any():
            raise ValueError("no position of xy_posns has a velocity inside the spectral axis")
        max_pos = max(0, int(np.ceil(np.nanmax(pix_shifts))))
        max_neg = min(0, int(np.ceil(np.nanmin(pix_shifts))))
        pad = (-max_neg, max_pos)
    return idx, pix_shifts, pad


def _finish(name, total, count, nnan, npos):
    with np.errstate(invalid="ignore", divide="ignore"):
        if name == "nanmean":
            return np.where(count > 0, total / count, np.nan)
        if name == "nansum":
            return total
        clean = np.where(nnan > 0, np.nan, total)
        return clean / npos if name == "mean" else clean


def _stack_sum_streamed(cube, idx, shifts, pad):
    """ops.stack_sum of a cube larger than the HBM budget: every row strip stacks the positions it holds, and the strips'
    sums and counts are added in strip order"""
    from . import streaming
    from .device import Stream
    nx = cube.shape[2]
    M = cube.shape[0] + pad[0] + pad[1]
    if M > _lib.STACK_MAX_CHANNELS:
        raise _lib.HipUnsupported("a padded spectrum of %d channels is above the built limit of %d" % (M, _lib.STACK_MAX_CHANNELS))
    total, count, nnan = np.zeros(M), np.zeros(M, np.int64), np.zeros(M, np.int64)
    nan_ex = _nan_term_dropped(cube, cube)
    compute = Stream(cube.device)
    rows = idx // nx
    for y0, y1, dev, mspec in streaming.Strips(cube, compute):
        sel = np.nonzero((rows >= y0) & (rows < y1))[0]
        if sel.size == 0:
            continue
        top = getattr(dev, "top", 0)
        t, c, n = ops.stack_sum(dev, idx[sel] - (y0 - top) * nx, shifts[sel], pad, fill=cube._fill_value, mask=mspec, stream=compute,
                                nan_excluded=nan_ex)
        total += t
        count += c
        nnan += n
    compute.synchronize()
    return total, count, nnan


def stack_spectra(cube, velocity_surface, v0=None, stack_function=np.nanmean, xy_posns=None, num_cores=1, chunk_size=-1,
                  progressbar=False, pad_edges=True, vdiff_tol=0.01):
    """Shift every spectrum of *cube* by *velocity_surface* (peak velocity, centroid, rotation model ...) to the common
    velocity *v0* and combine them with *stack_function* (analysis_utilities.py:134-318).

    *velocity_surface*: a (ny, nx) map; a plain array is in the cube's spectral unit, anything with ``.value`` and
    ``.unit`` (an astropy Quantity, the Projection ``cube.moment1()`` returns) is converted.  *v0*: the same for one
    number (a plain number is accepted here, the reference insists on a Quantity); the default is the mean of the
    spectral axis.  *xy_posns*: the positions to stack, as ``np.where`` returns them; the default is every finite
    velocity.  *pad_edges*: zero-pad every spectrum by the largest shifts so that nothing wraps around; the result then
    has ``nz + max_pos - max_neg`` channels and ``CRPIX1`` moved by ``-max_neg``.  *num_cores*, *chunk_size* and
    *progressbar* are accepted and ignored.

    Returns the stacked spectrum as a 1-D float64 ``Projection`` with the cube's unit, meta and beam(s) and the shifted
    spectral WCS.  The padded length may be at most 8192 channels.  A cube larger than the HBM budget runs strip by strip
    for np.nanmean / np.mean / np.nansum / np.sum; any other *stack_function* needs the shifted spectra ((P, M) float64)
    inside the budget, else ``HugeCubeError``."""
    from . import streaming
    idx, shifts, pad = stack_plan(cube, velocity_surface, v0=v0, xy_posns=xy_posns, pad_edges=pad_edges, vdiff_tol=vdiff_tol)
    nz = cube.shape[0]
    M = nz + pad[0] + pad[1]
    _lib.require_gpu()
    fused = _fused_name(stack_function)
    streamed = cube._stream_source() is not None
    if fused is not None and streamed:
        total, count, nnan = _stack_sum_streamed(cube, idx, shifts, pad)
        stacked = _finish(fused, total, count, nnan, idx.size)
    elif fused is not None:
        data, mask, view = cube._operand()
        total, count, nnan = ops.stack_sum(data, idx, shifts, pad, fill=cube._fill_value, mask=mask,
                                           nan_excluded=_nan_term_dropped(cube, view))
        stacked = _finish(fused, total, count, nnan, idx.size)
    else:
        need, budget = 8 * M * idx.size, streaming.hbm_budget(cube.device)
        if streamed or need > budget:
            raise streaming.HugeCubeError(
                "stack_function %r needs every shifted spectrum: %d x %d float64 (%.2f GiB) next to the whole cube in HBM, against "
                "a budget of %.2f GiB (SPC_HBM_BUDGET); np.nanmean, np.mean, np.nansum and np.sum stack without them"
                % (getattr(stack_function, "__name__", stack_function), idx.size, M, need / 2**30, budget / 2**30))
        data, mask, view = cube._operand()
        out = ops.stack_shift(data, idx, shifts, pad, fill=cube._fill_value, mask=mask, nan_excluded=_nan_term_dropped(cube, view))
        rows = np.ascontiguousarray(out.get().T)           # (P, M): what the reference hands to stack_function
        stacked = np.asarray(stack_function(rows, axis=0), dtype=np.float64)
    w1 = None
    if cube._wcs is not None:
        h = dict(cube._wcs.spectral_only().header)
        h["CRPIX1"] = float(h["CRPIX1"]) + pad[0]
        h["NAXIS1"] = int(M)
        w1 = SpectralAxisWCS(h)
    meta = dict(cube._meta or {})
    beam = None
    if hasattr(cube, "unmasked_beams"):
        meta["beams"] = list(cube.beams)
    else:
        beam = cube.beam
    spec = Projection(stacked, unit=cube._unit, wcs=w1, meta=meta, beam=beam, device=cube.device)
    if "beams" in meta:
        spec.beams = meta["beams"]
    return spec


# ---- stack_cube ---------------------------------------------------------------------------------------------------
C_KMS = 299792.458                       # km/s


class StackCubePlan:
    """what ``stack_cube_plan`` returns.  Per surviving (line, cube) pair, in the reference's order (lines outer, cubes
    inner): ``lines`` (the rest value as given), ``cube_index``, ``windows`` ((ilo, ihi), both ends included) and the rows
    of the (S, n0) tables ``lo`` (absolute lower channel, -1 = outside the slab), ``t``, ``inv_dx`` and ``exact`` of
    ``ops.stack_cube``; ``grid`` (n0 velocities, km/s), ``wcs`` (the output WCS), ``coarse`` (per source: the reference's
    SmoothingWarning condition holds)."""


def _speed_kms(value):
    if not hasattr(value, "unit"):
        return float(value)
    unit = value.unit
    unit = str(getattr(unit, "to_string", lambda: unit)()).replace(" ", "")
    if _SPECTRAL_SI.get(unit, (None,))[0] != "speed":
        raise UnitsError("vmin / vmax should be velocities (got %s)" % unit)
    return float(value.value) * spectral_unit_scale(unit, "km/s")


def _frequency_axis(cube):
    """the cube's channel frequencies (its spectral unit) after the checks of step 1: a linear FREQ axis in a unit of the
    Hz family; anything else is a change of representation that is not built"""
    w = cube._wcs
    ctype = str(w.ctype[2]).strip().upper() if w is not None and w.naxis >= 3 else ""
    kind = _SPECTRAL_SI.get(cube.spectral_unit, (None,))[0]
    if ctype != "FREQ" or kind != "freq":
        raise NotImplementedError("stack_cube needs a linear frequency axis (CTYPE3 = 'FREQ' in Hz, kHz, MHz or GHz): a %r axis in "
                                  "%r is not built (the reference converts it through its rest frequency)"
                                  % (ctype or "?", cube.spectral_unit))
    return np.asarray(cube.spectral_axis, dtype=np.float64)


def _lerp_rows(x, grid):
    """(lo, t, inv_dx, coarse) of one slab with axis *x* onto *grid*, lo relative to the slab's first channel: the plan of
    ops.lerp_plan turned to the slab's own channel order as SpectralCube.spectral_interpolate does"""
    lo, t, inv_dx, rin, rout, _ = ops.lerp_plan(x, grid)
    n = len(x)
    xs, gs = (x[::-1] if rin else x), (grid[::-1] if rout else grid)
    coarse = np.mean(np.diff(gs)) > 2 * np.mean(np.diff(xs))
    if rin:          # channel k of the sorted slab is channel n - 1 - k: interpolate from the upper neighbour downwards
        t = np.where(lo >= 0, xs[np.clip(lo, 0, n - 2) + 1] - gs, 0.0)
        lo = np.where(lo >= 0, n - 2 - lo, -1).astype(np.int32)
    if rout:
        lo, t, inv_dx = lo[::-1].copy(), t[::-1].copy(), inv_dx[::-1].copy()
    return lo, t, inv_dx, bool(coarse)


def stack_cube_plan(cube, linelist, vmin, vmax):
    """the host side of ``stack_cube`` up to the kernels (analysis_utilities.py:364-410): a StackCubePlan.  *cube*: one
    cube or a list of cubes of equal spatial shape."""
    cubes = list(cube) if isinstance(cube, (list, tuple)) else [cube]
    for cb in cubes[1:]:
        if tuple(cb.shape[1:]) != tuple(cubes[0].shape[1:]):
            raise ValueError("If you pass multiple cubes, they must have the same spatial shape.")
    vlo, vhi = _speed_kms(vmin), _speed_kms(vmax)
    freqs = [_frequency_axis(cb) for cb in cubes]
    for f in freqs:
        if f.size > 2 and not np.allclose(np.diff(f), f[1] - f[0], rtol=1e-9, atol=0.0):
            raise NotImplementedError("stack_cube needs a frequency axis that is linear in the channel number")
    P = StackCubePlan()
    P.lines, P.cube_index, P.windows, P.coarse = [], [], [], []
    axes = []
    for restval in linelist:
        for ci, cb in enumerate(cubes):
            f0 = float(_in_spectral_unit(cb, restval))
            v = C_KMS * (f0 - freqs[ci]) / f0
            a, b = int(np.argmin(np.abs(v - vlo))), int(np.argmin(np.abs(v - vhi)))
            ilo, ihi = min(a, b), max(a, b)
            if ihi - ilo + 1 <= 1:
                continue                                     # (a size-1 spectral axis: skipped, :388-391)
            P.lines.append(restval)
            P.cube_index.append(ci)
            P.windows.append((ilo, ihi))
            axes.append((f0, v))
    if not P.windows:
        raise ValueError("no line of the list has a slab of more than one channel between vmin and vmax in any cube")
    (ilo0, ihi0), (f00, v0), ref = P.windows[0], axes[0], cubes[P.cube_index[0]]
    P.grid = v0[ilo0:ihi0 + 1].copy()
    n0 = P.grid.size
    P.lo, P.t, P.inv_dx = np.full((len(axes), n0), -1, np.int32), np.zeros((len(axes), n0)), np.ones((len(axes), n0))
    P.exact = np.zeros(len(axes), np.int32)
    P.lo[0], P.exact[0] = ilo0 + np.arange(n0), 1
    P.coarse.append(False)
    for s in range(1, len(axes)):
        ilo, ihi = P.windows[s]
        lo, t, inv_dx, coarse = _lerp_rows(axes[s][1][ilo:ihi + 1], P.grid)
        P.lo[s], P.t[s], P.inv_dx[s] = np.where(lo >= 0, lo + ilo, -1), t, inv_dx
        P.coarse.append(coarse)
    w = ref._wcs
    sl = w.sliced((slice(ilo0, ihi0 + 1), slice(None), slice(None)), ref.shape)
    P.wcs = sl.with_spectral(C_KMS * (f00 - sl.crval[2]) / f00, -C_KMS * sl.cdelt[2] * sl.pc[2, 2] / f00, sl.crpix[2],
                             cunit="km/s", ctype="VRAD", drop_rest=True)
    return P


def _finite_cube(like, wcs, meta, data=None, dev=None, dev64=None):
    """a plain SpectralCube with the unit and fill value of *like* and the finite-value mask of a fresh cube"""
    from . import masks as M
    shape = tuple((data if data is not None else dev if dev is not None else dev64).shape)
    if dev64 is not None:
        out = like._new_wide_cube(lambda: dev64, shape=shape, wcs=wcs, mask=False, plain=True)
        out._meta = dict(meta)
    else:
        out = SpectralCube._new_cube_with(like, data=data, dev=dev, wcs=wcs, mask=False, meta=meta, shape=shape)
    out._mask = M.LazyMask(np.isfinite, cube=out)
    return out


def _cutouts(cubes, P, convolve_beam):
    """the cutouts of the general route as host arrays, each made on the device: the filled reference slab, and every
    other slab through ops.spectral_lerp with NaN replaced by the fill value (the filled data of a cube masked ~isnan)"""
    out = []
    for s, (ci, (ilo, ihi)) in enumerate(zip(P.cube_index, P.windows)):
        cb = cubes[ci]
        fill = cb._fill_value
        view = (slice(ilo, ihi + 1), slice(None), slice(None))
        rel = np.where(P.lo[s] >= 0, P.lo[s] - ilo, -1).astype(np.int32)
        if hasattr(cb, "unmasked_beams"):
            if convolve_beam is None:
                raise ValueError("If any of the input cubes have varying resolution, a target `convolve_beam` must be specified.")
            slab = cb[view].convolve_to(convolve_beam)
            if P.exact[s]:
                out.append(np.asarray(slab.filled_data))
                continue
            data, mask, _ = slab._operand()
        else:
            spec = cb._view_spec(view)
            shape = tuple(a[2] for a in spec)
            data, inc = cb._gather(spec, shape, filled=bool(P.exact[s]))
            if P.exact[s]:
                out.append(data.get())
                continue
            mask = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, inc) if inc is not None else None
        c = ops.spectral_lerp(data, rel, P.t[s], P.inv_dx[s], np.nan, mask=mask).get()
        out.append(np.where(np.isnan(c), c.dtype.type(fill), c))
    return out


def stack_cube(cube, linelist, vmin, vmax, average=np.nanmean, convolve_beam=None, return_hdu=False, return_cutouts=False):
    """Stack the spectral lines *linelist* of one wide-band frequency cube (or a list of cubes) into one cube on a common
    velocity grid (analysis_utilities.py:321-432).

    Per rest value (a plain number in the cube's spectral unit, or anything with ``.value`` / ``.unit`` in a frequency
    unit) the spectral axis becomes a radio velocity, ``v = c (f0 - f) / f0`` in km/s, and the slab between *vmin* and
    *vmax* (km/s, or speed quantities; either order, closest channels, both ends included) is cut; a slab of one channel
    is skipped.  The first surviving slab is taken as it is (filled) and gives the output grid, every other one is
    interpolated onto it as ``spectral_interpolate`` does (NaN outside the slab's own range and where a bracketing sample is
    NaN or masked; the interpolated slab is masked ~isnan, so those become the fill value), and ``average(cutouts, axis=0)``
    is the result: a plain SpectralCube on the device with the reference slab's celestial WCS, a 'VRAD' axis in km/s without
    a rest frequency, ``meta['stacked_lines']``, the cube's unit and fill value and a finite-value mask.

    The cube must have a linear 'FREQ' axis (NotImplementedError otherwise).  One resident cube with np.nanmean / np.mean /
    np.nansum / np.sum and ``return_cutouts=False`` runs in one kernel that writes no cutout; a list of cubes, any other
    *average*, ``return_cutouts=True`` (the list of host arrays is returned as well) and a varying-resolution cube with
    *convolve_beam* make every cutout on the device, fetch them and apply *average* on the host.  ``return_hdu=True``
    returns ``(header, filled array)`` instead of the cube.  An out-of-core cube raises HugeCubeError."""
    from . import streaming
    cubes = list(cube) if isinstance(cube, (list, tuple)) else [cube]
    is_list = isinstance(cube, (list, tuple))
    if not cubes:
        raise ValueError("an empty list of cubes")
    if is_list and convolve_beam is None and (any(hasattr(cb, "unmasked_beams") for cb in cubes)
                                              or not all(cb.beam == cubes[0].beam for cb in cubes[1:])):
        # (the spatial shapes are compared first, in stack_cube_plan - the reference's order)
        for cb in cubes[1:]:
            if tuple(cb.shape[1:]) != tuple(cubes[0].shape[1:]):
                raise ValueError("If you pass multiple cubes, they must have the same spatial shape.")
        raise ValueError("If the cubes have different resolution, `convolve_beam` must be specified.")
    P = stack_cube_plan(cubes, linelist, vmin, vmax)
    nsrc, n0 = P.lo.shape
    fused = _fused_name(average)
    varying = any(hasattr(cb, "unmasked_beams") for cb in cubes)
    one_kernel = fused is not None and not is_list and not return_cutouts and not varying
    if one_kernel and nsrc > _lib.STACK_CUBE_MAX_LINES:
        raise _lib.HipUnsupported("%d lines are above the built limit of %d for one pass (STACK_CUBE_MAX_LINES); another "
                                  "`average` or return_cutouts=True takes the route that makes every cutout"
                                  % (nsrc, _lib.STACK_CUBE_MAX_LINES))
    for cb in cubes:
        if cb._stream_source() is not None:
            raise streaming.HugeCubeError("stack_cube needs the cube resident in HBM: %s is larger than the budget "
                                          "(SPC_HBM_BUDGET) and strip streaming is not built for stack_cube" % (cb.shape,))
    if any(P.coarse):
        warnings.warn("Input grid has too small a spacing. The data should be smoothed prior to resampling.", SmoothingWarning,
                      stacklevel=2)
    ref = cubes[P.cube_index[0]]
    meta = dict(ref._meta or {})
    meta["stacked_lines"] = list(P.lines)
    _lib.require_gpu()
    cutouts = None
    if one_kernel:
        data, mask, view = ref._operand()
        out = ops.stack_cube(data, P.lo, P.t, P.inv_dx, P.exact, fused, fill=ref._fill_value, mask=mask,
                             nan_excluded=_nan_term_dropped(ref, view))
        wide = out.dtype == np.float64
        result = _finite_cube(ref, P.wcs, meta, dev=None if wide else out, dev64=out if wide else None)
    else:
        ny, nx = ref.shape[1:]
        need, budget = 2 * 8 * nsrc * n0 * ny * nx, streaming.hbm_budget(ref.device)
        if need > budget:
            raise streaming.HugeCubeError(
                "stack_cube with average %r makes every cutout: %d x (%d, %d, %d) (%.2f GiB on the device and on the host) against "
                "a budget of %.2f GiB (SPC_HBM_BUDGET); np.nanmean, np.mean, np.nansum and np.sum of one cube stack without them"
                % (getattr(average, "__name__", average), nsrc, n0, ny, nx, need / 2**30, budget / 2**30))
        cutouts = _cutouts(cubes, P, convolve_beam)
        stacked = np.asarray(average(cutouts, axis=0))
        dtype = np.float64 if ref._runs_wide() else np.float32
        result = _finite_cube(ref, P.wcs, meta, data=np.ascontiguousarray(stacked, dtype=dtype))
    retval = (dict(result.header), np.asarray(result.filled_data)) if return_hdu else result
    return (retval, cutouts) if return_cutouts else retval
