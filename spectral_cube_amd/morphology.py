"""Binary morphology of cube masks on the device: dilate, erode, open, close, propagate.

What users of the reference do on the host with ``scipy.ndimage.binary_dilation`` / ``binary_erosion`` /
``binary_opening`` / ``binary_closing`` / ``binary_propagation`` on ``cube.get_mask_array()`` (spectral_cube.py:552),
here on the uint8 include array where it lives (ops.mask_morph, csrc/spc_mask_morph.hip): the result is a
:class:`~spectral_cube_amd.masks.DeviceBooleanMask` that goes straight into ``cube.with_mask(...)``; no cube-sized array
travels to the host.  Every function follows the keywords of its scipy.ndimage namesake (scipy itself is never imported):

  * the structure's centre is ``size // 2`` on every axis, for even extents too; dilation is
    ``out[p] = OR over the offsets o of in[p - o]``, erosion ``out[p] = AND over o of in[p + o]``, samples outside the
    array are ``border_value``;
  * with ``mask``, ``out[p] = mask[p] ? result[p] : in[p]`` at every iteration;
  * ``iterations >= 1``: that many steps; ``iterations < 1``: until a step changes nothing.

The numpy restatement of these rules (tests/morphology.py) equals scipy.ndimage 1.15 on asymmetric and hollow structures,
even extents, ``border_value=1``, erosion under a mask and structures taller than the axis: no difference was found.

Limits: a structure is 3-D with every extent from 1 to 7 (a 2-D one is applied per plane, a 1-D one is refused);
``origin`` must be 0; ``brute_force`` and ``output`` are not accepted; an out-of-core cube is refused (propagation crosses
its strips).  A structure without its centre can cycle when it is repeated to a fixed point, in scipy for ever; here the
call ends with NotImplementedError after 65536 steps.
"""
import ctypes as C

import numpy as np

from . import _lib, ops
from . import masks as M
from .device import DeviceArray

MAX_EXTENT = 2 * _lib.MORPH_MAX_REACH + 1


def generate_binary_structure(rank, connectivity):
    """scipy.ndimage.generate_binary_structure: the 3**rank box, True within *connectivity* orthogonal steps of its centre"""
    connectivity = max(int(connectivity), 1)
    if rank < 1:
        return np.array(True, dtype=bool)
    return np.add.reduce(np.fabs(np.indices([3] * int(rank)) - 1), 0) <= connectivity


def _offsets(structure, origin):
    """(n, 3) int8: index - size // 2 of the True entries of *structure* as (nz, ny, nx) morphology takes it"""
    if np.any(np.asarray(origin) != 0):
        raise NotImplementedError("origin must be 0: a shifted structure is not built (shift the structure's entries instead)")
    if structure is None:
        structure = generate_binary_structure(3, 1)
    s = np.asarray(structure).astype(bool)
    if s.ndim == 1:
        raise ValueError("a 1-D structure does not say which axis it runs along: write structure.reshape(-1, 1, 1) for the "
                         "spectral axis, reshape(1, -1, 1) for y or reshape(1, 1, -1) for x")
    if s.ndim == 2:
        s = s[None]                                   # per plane
    if s.ndim != 3:
        raise ValueError("structure must have 2 or 3 dimensions (got %d)" % s.ndim)
    if s.size == 0 or not s.any():
        raise ValueError("structure must not be empty")
    if max(s.shape) > MAX_EXTENT:
        raise ValueError("structure of shape %s: every extent must be 1 to %d" % (s.shape, MAX_EXTENT))
    return (np.argwhere(s) - np.array(s.shape) // 2).astype(np.int8)


def _is_cube(x):
    return hasattr(x, "_operand") and hasattr(x, "_stream_source")


def _source(x, cube, what, fallback=None):
    """(shape, wcs, cube or None, fetch) of an input or a mask: the cube whose include map it is, if any, and
    fetch(device), which gives its uint8 DeviceArray (*device*: where a host array is uploaded).  Nothing touches the
    device before fetch()."""
    if _is_cube(x):
        return tuple(x.shape), x.wcs, x, lambda device: _cube_include(x)
    if isinstance(x, M.DeviceBooleanMask):
        return tuple(x.shape), x._wcs, None, lambda device: x.device_array()
    if isinstance(x, M.MaskBase):
        owner = cube if cube is not None else (M.foreign_owner(x) or fallback)      # `cube > 3` knows its cube
        if owner is None or not _is_cube(owner):
            raise TypeError("%s is a %s: pass cube= so that it can be evaluated" % (what, type(x).__name__))
        return _source(owner.with_mask(x, inherit_mask=False), None, what)
    a = np.asarray(x)
    if a.ndim != 3:
        raise ValueError("%s must be a cube, a mask or a bool array of shape (nz, ny, nx) (got shape %s)" % (what, a.shape))
    return (tuple(a.shape), cube.wcs if cube is not None else None, None,
            lambda device: DeviceArray.from_numpy(a != 0, device, dtype=np.uint8))


def _cube_include(cube):
    """the include map of *cube* as a uint8 DeviceArray: what get_mask_array() brings to the host, left where it is"""
    from .cube import _nan_term_dropped
    if cube._mask is None:
        out = DeviceArray(cube.shape, np.uint8, cube.device)
        _lib.call("spc_memset", cube.device, C.c_void_p(out.ptr), 1, out.nbytes, None)
        return out
    data, mspec, view = cube._operand()
    nan_ex = _nan_term_dropped(cube, view)
    if mspec.flags == _lib.MASK_ARRAY and not nan_ex:
        return mspec.array
    return ops.mask_include(data, mspec, nan_excluded=nan_ex)


def _run(steps, input, structure, iterations, mask, border_value, origin, cube):
    """*steps*: the ops run one after the other on the result of the one before (opening = erode, dilate)"""
    offs = _offsets(structure, origin)
    if border_value not in (0, 1, False, True):
        raise ValueError("border_value must be 0 or 1 (got %r)" % (border_value,))
    shape, wcs, owner, fetch = _source(input, cube, "input")
    owners, fetch_mask = [owner], None
    if mask is not None:
        mshape, _, mowner, fetch_mask = _source(mask, cube, "mask", fallback=owner)
        if mshape != shape:
            raise ValueError("mask of shape %s does not match the input's %s" % (mshape, shape))
        owners.append(mowner)
    for c in owners:
        if c is not None and c._stream_source() is not None:
            raise NotImplementedError("morphology needs the whole include map in HBM: an out-of-core cube is refused "
                                      "(propagation crosses its strips)")
    cur = fetch(cube.device if cube is not None else 0)
    m = fetch_mask(cur.device) if fetch_mask is not None else None
    for op in steps:
        cur = ops.mask_morph(cur, offs, op, iterations=int(iterations), mask=m, border_value=int(border_value))
    return M.DeviceBooleanMask(cur, wcs=wcs, shape=shape)


def binary_dilation(input, structure=None, iterations=1, mask=None, border_value=0, origin=0, cube=None):
    """scipy.ndimage.binary_dilation of a mask on the device.  *input* / *mask*: a SpectralCube (its include map, all True
    without a mask), a DeviceBooleanMask, any other mask together with *cube* = the cube it is evaluated on (a mask whose
    lazy terms all belong to one cube, ``cube > 3``, finds it itself), or a host bool array of shape (nz, ny, nx).
    Returns a DeviceBooleanMask with the input's WCS and shape."""
    return _run((_lib.MORPH_DILATE,), input, structure, iterations, mask, border_value, origin, cube)


def binary_erosion(input, structure=None, iterations=1, mask=None, border_value=0, origin=0, cube=None):
    """scipy.ndimage.binary_erosion of a mask on the device (inputs and result as for binary_dilation)"""
    return _run((_lib.MORPH_ERODE,), input, structure, iterations, mask, border_value, origin, cube)


def binary_opening(input, structure=None, iterations=1, mask=None, border_value=0, origin=0, cube=None):
    """scipy.ndimage.binary_opening: erosion, then dilation, both with the same *iterations*, *mask* and *border_value*"""
    return _run((_lib.MORPH_ERODE, _lib.MORPH_DILATE), input, structure, iterations, mask, border_value, origin, cube)


def binary_closing(input, structure=None, iterations=1, mask=None, border_value=0, origin=0, cube=None):
    """scipy.ndimage.binary_closing: dilation, then erosion, both with the same *iterations*, *mask* and *border_value*"""
    return _run((_lib.MORPH_DILATE, _lib.MORPH_ERODE), input, structure, iterations, mask, border_value, origin, cube)


def binary_propagation(input, structure=None, mask=None, border_value=0, origin=0, cube=None):
    """scipy.ndimage.binary_propagation: binary_dilation(..., iterations=-1, mask=mask), *input* grown into the connected
    part of *mask* (the least fixed point: the sweeps run in place, tile by tile, until one changes nothing)"""
    return _run((_lib.MORPH_DILATE,), input, structure, -1, mask, border_value, origin, cube)
