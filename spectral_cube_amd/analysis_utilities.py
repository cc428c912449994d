"""``stack_spectra`` of spectral_cube.analysis_utilities (analysis_utilities.py:134-318) on the device: every spectrum is
Fourier-shifted by its own number of channels so that the lines align, and the shifted spectra are combined into one.

The host restates the reference's bookkeeping (validation, default positions and ``v0``, the linearity check, the range
masking, the pixel shifts, the padding and the new ``CRPIX1`` / ``NAXIS1``) in its order; every voxel is touched only by
the HIP kernels of spc_stack.hip.  ``np.nanmean`` / ``np.mean`` / ``np.nansum`` / ``np.sum`` never write a shifted spectrum
(``ops.stack_sum``); any other ``stack_function`` receives the ``(P, M)`` array of shifted spectra (``ops.stack_shift``)
on the host, as in the reference.  There is no CPU fallback.
"""
import warnings

import numpy as np

from . import _lib, ops
from .cube import Projection, _nan_term_dropped
from .wcs import SpectralAxisWCS


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
