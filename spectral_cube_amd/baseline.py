"""Polynomial baselines on the device: fit a low-order polynomial to the line-free channels of every spectrum of a cube and
subtract it (ops.baseline_fit / ops.baseline_apply, spc_baseline_fit_f32 / _f64 and spc_baseline_apply_f32 / _f64).

The reference documents continuum subtraction for a constant only (docs/continuum_subtraction.rst: mask the line channels,
``median(axis=0)``, subtract); a slope or a ripple - a single-dish baseline, a spectral index across the band, CASA's
``imcontsub fitorder=n`` - goes through ``apply_function_parallel_spectral`` there, one Python call per spectrum on the
host.  Here the fit is one masked streaming pass over the cube and the subtraction one element-wise pass::

    signal = cube > 5 * noise                          # or the dilated / pruned mask of the morphology step
    fit = cube.fit_baseline(order=2, fit_mask=~signal, exclude=[(-30, 40)])
    flat = fit.subtract()                              # == cube.subtract_baseline(order=2, fit_mask=..., exclude=...)
    fit.continuum()                                    # Projection: the model at the band centre

The basis is Legendre on the channel index mapped to [-1, 1]; see include/spcube_hip.h for the arithmetic.  Not built:
iterative sigma-clipped refits (fit, build a mask from ``fit.subtract()``, fit again), weights, orders above 5, and a
basis in velocity rather than channel number (``polynomial()`` is in channels)."""
import numpy as np

from . import _lib, ops

MAX_ORDER = _lib.BASELINE_MAX_ORDER


def _check_order(order):
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or not 0 <= int(order) <= MAX_ORDER:
        raise ValueError("order must be an integer from 0 to %d (got %r): higher orders are not built" % (MAX_ORDER, order))
    return int(order)


def resolve_channels(cube, channels=None, exclude=None):
    """the increasing int32 channel numbers a fit of *cube* may use: *channels* (None: all; a boolean (nz,) array or integer
    indices) minus the channels of every ``(lo, hi)`` range of *exclude*, given in the cube's spectral unit (plain numbers,
    or objects with ``.value`` and ``.unit``) and resolved as spectral_slab resolves its limits - the closest channel to
    each end, both ends included, whichever way the spectral axis runs.  ValueError for bad indices and for lo > hi."""
    nz = int(cube.shape[0])
    chan = ops.baseline_channels(channels, nz)
    if exclude is None:
        return chan
    keep = np.zeros(nz, bool)
    keep[chan] = True
    ranges = list(exclude)
    if len(ranges) == 2 and not any(isinstance(r, (tuple, list, np.ndarray)) for r in ranges):
        raise ValueError("exclude must be a list of (lo, hi) ranges, e.g. [(lo, hi)]")
    for r in ranges:
        if len(r) != 2:
            raise ValueError("exclude must be a list of (lo, hi) ranges (got %r)" % (r,))
        lo, hi = cube._spectral_value(r[0]), cube._spectral_value(r[1])
        if not lo <= hi:
            raise ValueError("exclude range (%r, %r): lo must not be above hi" % (r[0], r[1]))
        ilo, ihi = cube.closest_spectral_channel(lo), cube.closest_spectral_channel(hi)
        if ilo > ihi:
            ilo, ihi = ihi, ilo
        keep[ilo:ihi + 1] = False
    return np.flatnonzero(keep).astype(np.int32)


class BaselineFit:
    """The baselines of a cube: one polynomial of degree ``order`` per spectrum.

    ``order``; ``coefficients``: the float64 ``(order + 1, ny, nx)`` DeviceArray of Legendre coefficients on the channel
    index mapped to [-1, 1]; ``channels``: the channel numbers the fit could use; ``npts``: how many samples each spectrum's
    fit did use (an int Projection; a spectrum with fewer than ``order + 1`` has NaN coefficients)."""

    def __init__(self, cube, order, coefficients, npts, channels):
        self.cube = cube
        self.order = int(order)
        self.coefficients = coefficients
        self.channels = channels
        self._npts_dev = npts
        self._npts = None

    def _projection(self, arr, unit, **meta):
        from .cube import Projection, VaryingResolutionSpectralCube
        cube = self.cube
        full = dict(cube.meta)
        full.update(baseline_order=self.order, **meta)
        beam = None if isinstance(cube, VaryingResolutionSpectralCube) else cube.beam
        return Projection(arr, unit=unit, wcs=cube.wcs.drop_spectral() if cube.wcs is not None else None, meta=full, beam=beam,
                          device=cube.device)

    @property
    def npts(self):
        if self._npts is None:
            self._npts = self._projection(self._npts_dev.get(), "")
        return self._npts

    def legendre(self):
        """host copy of the Legendre coefficients, float64 ``(order + 1, ny, nx)``"""
        return self.coefficients.get()

    def polynomial(self):
        """float64 ``(order + 1, ny, nx)``: the coefficients of 1, k, k^2 ... in the CHANNEL NUMBER k (lowest power first,
        numpy.polynomial's order; ``np.polyfit`` lists them the other way round), converted on the host.  The power basis
        is badly conditioned on long axes at high order: evaluate ``legendre()`` where accuracy matters."""
        P = np.polynomial
        leg = self.legendre()
        nz, nc = int(self.cube.shape[0]), self.order + 1
        to_t = np.zeros((nc, nc))                    # column j: P_j as a power series in t
        for j in range(nc):
            to_t[:j + 1, j] = P.legendre.leg2poly(np.eye(nc)[j][:j + 1])
        a, b = (2.0 / (nz - 1), -1.0) if nz > 1 else (0.0, 0.0)       # t = a k + b
        to_k = np.zeros((nc, nc))                    # column j: t^j as a power series in k
        power = np.ones(1)
        for j in range(nc):
            to_k[:j + 1, j] = power
            power = np.convolve(power, [b, a])
        return np.tensordot(to_k @ to_t, leg, axes=(1, 0))

    def continuum(self, channel=None):
        """Projection in the cube's unit: the model at *channel* (a channel number, fractional ones allowed); None: the band
        centre, t = 0.  Evaluated on the host from ``legendre()``."""
        nz = int(self.cube.shape[0])
        if channel is None:
            t = 0.0
        else:
            t = (2.0 * float(channel) - (nz - 1)) / (nz - 1) if nz > 1 else 0.0
        row = np.polynomial.legendre.legvander(np.array([t]), self.order)[0]
        return self._projection(np.tensordot(row, self.legendre(), axes=(0, 0)), self.cube.unit,
                                baseline_channel=None if channel is None else float(channel))

    def _applied(self, subtract):
        coef = self.coefficients
        return self.cube._derived(lambda data, mspec, view: ops.baseline_apply(data, coef, subtract=subtract))

    def model(self):
        """SpectralCube (the cube's own class, mask - not the fit mask -, WCS, unit, meta and beam(s)): the baseline model in
        every voxel"""
        return self._applied(False)

    def subtract(self):
        """SpectralCube like ``model()``: the cube minus its baselines, in every voxel whatever the masks say (as
        ``cube - map`` treats the unmasked data); a spectrum that could not be fitted comes out NaN"""
        return self._applied(True)


def fit_baseline(cube, order=1, fit_mask=None, channels=None, exclude=None):
    """:class:`BaselineFit` of *cube*: a polynomial of degree *order* (0 ... 5) fitted by least squares to every spectrum
    on the device.  A spectrum is fitted on the channels that *channels* (a boolean (nz,) array or integer indices; None:
    all) names, that no ``(lo, hi)`` range of *exclude* (spectral coordinates, both ends included) covers, whose voxel the
    mask of ``cube.with_mask(fit_mask)`` includes (*fit_mask*: anything with_mask accepts, ``~signal`` being the intended
    use; None: the cube's own mask) and whose sample is not NaN.  ValueError for an order that is no integer in 0 ... 5,
    bad channel indices, lo > hi and fewer than ``order + 1`` channels; NotImplementedError for a cube larger than the HBM
    budget.  A cube with pending arithmetic is materialised first."""
    order = _check_order(order)
    chan = resolve_channels(cube, channels, exclude)
    if chan.size < order + 1:
        raise ValueError("a fit of order %d needs at least %d channels and %d are left" % (order, order + 1, chan.size))
    if cube._stream_source() is not None:
        raise NotImplementedError("fitting baselines needs the whole cube in HBM: an out-of-core cube is refused (cut it "
                                  "first - cube[:, y0:y1, x0:x1] streams only what it touches - and fit the cut)")
    masked = cube if fit_mask is None else cube.with_mask(fit_mask)
    data, mspec, _ = masked._operand()
    all_channels = chan.size == int(cube.shape[0])
    coef, npts = ops.baseline_fit(data, order, channels=None if all_channels else chan,
                                  mask_spec=mspec if masked._mask is not None else None)
    return BaselineFit(cube, order, coef, npts, chan)


def subtract_baseline(cube, order=1, fit_mask=None, channels=None, exclude=None):
    """``fit_baseline(cube, ...).subtract()``: the cube minus a polynomial baseline of degree *order* per spectrum"""
    return fit_baseline(cube, order=order, fit_mask=fit_mask, channels=channels, exclude=exclude).subtract()
