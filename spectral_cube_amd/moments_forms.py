"""The forms in which moments() reads a reused mask and cube, and the ladder that chooses between them.

A MaskSpec (ops.py) that is used again is taken to describe the same mask.  select() climbs one rung per use, under one hold of
the lock, and names the entry point the launch goes to:

1. spc_moments_f32, the bytes.  A spec's first use costs what it always did.
2. spc_moments_bits_f32.  From its second use on the array term is read as bits (spc_mask_pack_bits: an eighth of the bytes per
   launch), packed once and kept with the spec.  The bits are keyed by the array's address, shape, strides and WRITE GENERATION
   (DeviceArray.mark_written: upload() and every operator of this package that writes into a caller-given array advance it), so
   a mask rewritten that way is packed again after two more uses.  Bytes changed behind the library's back - through the raw
   pointer, by a kernel of the caller's - after a spec has been used twice need MaskSpec.invalidate().  rows(), planes() and
   swap01() return specs of their own, which pack for themselves on their second use.  SPC_MOMENTS_MASK_BITS=0 turns the bits off.
3. spc_moments_list_f32.  A spec that is used again ON THE SAME CUBE goes one step further: the launch that finds the bits packed
   by an earlier call and the cube of the launch before it (normally the third use) builds the list of the cube's 16-byte lane
   segments that the bits include (spc_moments_list_*: include/spcube_hip.h) and later launches with the same launch plan read
   that list instead of marching the cube - where the list is at most half of the bytes the march fetches (list_is_kept);
   otherwise it is refused, once, and the march goes on.  The list costs 1280 bytes of HBM per entry row (about 14 GB for a
   4096 x 2048 x 2048 cube under a 4 % mask) and lives as long as the spec.  It is keyed by the bits' key and the cube's root
   array BY IDENTITY (a weak reference: a freed cube whose address a new array reuses never matches), its address, shape,
   strides and write generation: another cube, upload() into the cube or an operator of this package writing into it (out=,
   scale_inplace) drop the list - the voxel list with it - and only them.  SAMPLES changed behind the library's back after a
   spec's second use on the cube need invalidate() just as mask bytes do.  SPC_MOMENTS_LIST=0 turns the list off.
4. spc_moments_vlist_f32.  The launch that finds a non-empty list built by an earlier call (normally the fourth use) compacts it
   into the VOXEL list (spc_moments_vlist_*): one 8-byte entry per included voxel instead of a 20-byte entry per included lane
   segment, kept only where it reads at most half of what the list does (vlist_is_kept: masks that keep about one voxel of a
   segment; connected masks are refused, once, and stay on the list).  The list's arrays stay allocated beside it (6 GB of voxel
   list beside 14 GB of list for that cube).  SPC_MOMENTS_VLIST=0 turns the voxel list off, and is remembered on the spec.

A launch that builds a form works on the caller's stream and waits for it once, so that later launches on any stream may read
what was built, and then uses it.  A refusal, a launch the library has no such form for and a failed allocation are remembered
on the spec and are silent: the launch goes to the rung below.  Whether a launch's plan can read what it is given is the
library's decision (moments_run, csrc/spc_moments.hip)."""
import ctypes as C
import os
import threading
import weakref

import numpy as np

from . import _lib
from .device import DeviceArray, _sh

_bits_lock = threading.Lock()        # dask `threads` workers share a spec: one of them builds


def _switch_on(name, dflt=1):
    """a library switch as spc_switch reads it: atoi of the value when set ("" and text that is no number: 0)"""
    e = os.environ.get(name)
    if e is None:
        return dflt != 0
    e = e.strip()
    n = 0
    while n < len(e) and (e[n].isdigit() or (n == 0 and e[n] in "+-")):
        n += 1
    try:
        return int(e[:n]) != 0
    except ValueError:
        return False


class _MomentsList:
    """the device arrays of one list (spc_moments_list: include/spcube_hip.h) and the struct that names them"""

    def __init__(self, desc, off, length, samples, meta, rows):
        self.desc, self.off, self.len, self.samples, self.meta, self.rows = desc, off, length, samples, meta, int(rows)
        c = self.c = _lib.SpcMomentsList()
        c.desc = desc
        c.d_samples, c.samples_bytes = samples.ptr, samples.nbytes
        c.d_meta, c.meta_bytes = meta.ptr, meta.nbytes
        c.d_off, c.d_len, c.nsublists = off.ptr, length.ptr, int(desc.nblocks * desc.nsub)
        c.rows = self.rows

    @property
    def nbytes(self):
        return self.rows * 1280


class _MomentsVlist:
    """the device arrays of one voxel list (spc_moments_vlist: include/spcube_hip.h) and the struct that names them"""

    def __init__(self, desc, off, length, entries, rows):
        self.desc, self.off, self.len, self.entries, self.rows = desc, off, length, entries, int(rows)
        c = self.c = _lib.SpcMomentsVlist()
        c.desc = desc
        c.d_entries, c.entries_bytes = entries.ptr, entries.nbytes
        c.d_off, c.d_len, c.nsublists = off.ptr, length.ptr, int(desc.nblocks * desc.nsub)
        c.rows = self.rows

    @property
    def nbytes(self):
        return self.rows * 512


def list_is_kept(rows, lines, nblocks, nz):
    """the list is built only where it reads at most half of what the bits march fetches: 1280 bytes per entry row against
    128 per fetched cube line and 32 of bits per block and plane.  A condition, not a tuning result: all-ones and dense
    random masks stay with the march"""
    return 2 * 1280 * int(rows) <= 128 * int(lines) + 32 * int(nblocks) * int(nz)


def vlist_is_kept(vrows, rows):
    """the voxel list is kept only where it reads at most half of what the list it is made from does: 512 bytes per entry row
    against 1280.  A condition, not a tuning result: masks that keep three or four voxels of a lane segment (connected
    signal masks) stay on the list"""
    return 2 * 512 * int(vrows) <= 1280 * int(rows)


def _cube_key(cube):
    nz, ny, nx = cube.shape
    return (cube.ptr, cube.shape, getattr(cube, "row_stride", nx), getattr(cube, "plane_stride", ny * nx), cube.write_generation)


def _pack(mask, need, stream):
    """the array term of *mask* as *need* bytes of bits, or None where that form does not exist (*need* is 0)"""
    a = mask.array
    if not need:
        return None
    bits = DeviceArray((need,), np.uint8, a.device)
    m = mask.to_c()
    _lib.call("spc_mask_pack_bits", a.device, _sh(stream), *a.shape, C.byref(m), C.c_void_p(bits.ptr), need)
    _lib.call("spc_stream_sync", a.device, _sh(stream))
    return bits


def _build_list(cube, bits, stream, c, m, o, ws):
    """the list of *cube*'s lane segments that *bits* include, for the plan of this launch, or None where list_is_kept refuses it:
    counted, the offsets formed on the host, allocated, filled"""
    bp = (C.c_void_p(bits.ptr), bits.nbytes)
    desc = _lib.SpcMomentsListDesc()
    _lib.call("spc_moments_list_plan_f32", C.byref(c), C.byref(m), C.byref(o), *ws, C.byref(desc))
    n = int(desc.nblocks * desc.nsub)
    d_len, d_lines = DeviceArray((n,), np.uint32, cube.device), DeviceArray((n,), np.uint32, cube.device)
    _lib.call("spc_moments_list_count_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), C.byref(o), *ws, *bp,
              C.c_void_p(d_len.ptr), C.c_void_p(d_lines.ptr), n, C.byref(desc))
    length = d_len.get(stream).astype(np.uint64)               # (waits for the stream)
    lines = int(d_lines.get(stream).astype(np.uint64).sum())
    rows = int(length.sum())
    if not list_is_kept(rows, lines, desc.nblocks, cube.shape[0]):
        return None
    off = DeviceArray.from_numpy(np.cumsum(length) - length, cube.device, stream)
    samples = DeviceArray((max(rows, 1) * 1024,), np.uint8, cube.device)
    meta = DeviceArray((max(rows, 1) * 256,), np.uint8, cube.device)
    lst = _MomentsList(desc, off, d_len, samples, meta, rows)
    _lib.call("spc_moments_list_fill_f32", cube.device, _sh(stream), C.byref(c), *bp, C.byref(lst.c))
    _lib.call("spc_stream_sync", cube.device, _sh(stream))
    return lst


def _build_vlist(lst, device, stream):
    """the voxel list made from *lst*, or None where vlist_is_kept refuses it: counted, the offsets formed on the host, allocated,
    filled"""
    n = int(lst.desc.nblocks * lst.desc.nsub)
    d_vlen = DeviceArray((n,), np.uint32, device)
    _lib.call("spc_moments_vlist_count_f32", device, _sh(stream), C.byref(lst.c), C.c_void_p(d_vlen.ptr), n)
    vlen = d_vlen.get(stream).astype(np.uint64)                # (waits for the stream)
    vrows = int(vlen.sum())
    if not vlist_is_kept(vrows, lst.rows):
        return None
    voff = DeviceArray.from_numpy(np.cumsum(vlen) - vlen, device, stream)
    entries = DeviceArray((max(vrows, 1) * 512,), np.uint8, device)
    vl = _MomentsVlist(lst.desc, voff, d_vlen, entries, vrows)
    _lib.call("spc_moments_vlist_fill_f32", device, _sh(stream), C.byref(lst.c), C.byref(vl.c))
    _lib.call("spc_stream_sync", device, _sh(stream))
    return vl


def _kept(mask, slot, build):
    """what *build*() makes, kept in the spec's *slot*.  None (a refusal, no such form), an error of the library and a failed
    allocation set <slot>_failed instead and are never an error: the launch goes to the rung below and does not ask again"""
    try:
        made = build()
    except (_lib.HipLibraryError, _lib.HipUnsupported, MemoryError):
        made = None
    if made is None:
        setattr(mask, slot + "_failed", True)
    else:
        setattr(mask, slot, made)
    return made


def select(mask, cube, stream, c, m, o, ws):
    """(entry point, the arguments that follow its common ten, the objects those arguments point into) of this launch of
    moments(): *c*, *m*, *o* are the structs of the cube, the mask and the outputs, *ws* the (pointer, bytes) of the workspace.
    Builds at most one form per rung (the module's docstring has the rules) and holds the lock throughout, so nothing is
    dropped between the rungs.  The arguments are raw addresses: THE CALLER HOLDS THE THIRD ITEM UNTIL ITS _lib.call HAS
    RETURNED - the lock is released here, and a drop in another thread (another cube, a changed write generation, invalidate())
    may then take the spec's last reference to the bits, the list or the voxel list; freed after the launch is queued, spc_free
    waits for it, freed before, the launch would read memory that is no longer theirs"""
    if mask is None or mask.array is None:
        return "spc_moments_f32", (), ()
    a = mask.array
    root = cube._root() if isinstance(cube, DeviceArray) else None
    with _bits_lock:
        bits = packed_before = None
        if mask.flags & _lib.MASK_ARRAY and len(a.shape) == 3 and _switch_on("SPC_MOMENTS_MASK_BITS"):
            key = _cube_key(a)
            if mask._bits_key != key:
                mask._drop_bits()
                mask._bits_key = key
            bits = packed_before = mask._bits
            if bits is None and not mask._bits_failed:
                mask._bits_uses += 1
                if mask._bits_uses >= 2:
                    need = int(_lib.load().spc_mask_bits_bytes(*a.shape))
                    bits = _kept(mask, "_bits", lambda: _pack(mask, need, stream))
        lst = built_before = None
        if root is not None:
            key = (mask._bits_key,) + _cube_key(cube)
            if mask._list_key == key and mask._list_root is not None and mask._list_root() is root:
                lst = built_before = mask._list
                if lst is None and not mask._list_failed and packed_before is not None and _switch_on("SPC_MOMENTS_LIST"):
                    lst = _kept(mask, "_list", lambda: _build_list(cube, bits, stream, c, m, o, ws))
            else:                            # not the cube of the launch before: that launch is this one now
                mask._drop_list()
                mask._list_key, mask._list_root = key, weakref.ref(root)
        if bits is None:
            return "spc_moments_f32", (), ()
        extra = (C.c_void_p(bits.ptr), bits.nbytes)
        if lst is None:
            return "spc_moments_bits_f32", extra, (bits,)
        extra += (C.byref(lst.c),)
        vl = mask._vlist
        if vl is None and not mask._vlist_failed and built_before is lst and lst.rows:     # an empty list is never compacted
            if _switch_on("SPC_MOMENTS_VLIST"):
                vl = _kept(mask, "_vlist", lambda: _build_vlist(lst, cube.device, stream))
            else:
                mask._vlist_failed = True
        if vl is None:
            return "spc_moments_list_f32", extra, (bits, lst)
        return "spc_moments_vlist_f32", extra + (C.byref(vl.c),), (bits, lst, vl)
