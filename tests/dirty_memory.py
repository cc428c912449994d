"""What device memory held before the call: shared by test_gpu_dirty_memory.py (GPU) and test_dirty_memory_host.py (CPU).

``ops.workspace()`` keeps one grow-only scratch buffer per (device, stream, thread), so every entry point that takes a
``d_workspace`` starts on the leftovers of the operator before it, and ``spc_malloc`` hands freed blocks out again, so a
fresh ``DeviceArray`` - an output, a per-call workspace, a table - is a recycled block.  The contract (docs/DESIGN_NOTES.md,
"What memory an entry may assume"): scratch and fresh outputs arrive dirty, an entry initialises what it reads.  The oracle
needs no tolerance: a result must not depend on what that memory held.

``dirty(pattern)`` fills every cached scratch buffer and, while it is open, every owning allocation with one of PATTERNS:

  pattern    float32 / float64      integers             flag / mask byte
  0x00       0.0                    0                    clear
  0xFF       NaN                    -1 / all ones        set
  0x7F       3.39e38 / 1.4e306      2139062143           127
  "random"   bytes of np.random.default_rng(seed + allocation counter), uploaded

One pattern hides half the ways to depend on memory: a sum that accumulates into uncleared scratch is right on 0x00, a
status byte read as "done" when nonzero is right (or uniformly wrong) on 0xFF and 0x7F - test_dirty_memory_host.py shows
both on a toy operator.  Importing this module touches no GPU."""
import contextlib
import ctypes as C

import numpy as np

from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray

PATTERNS = (0x00, 0xFF, 0x7F, "random")
SEED = 20261019


def pattern_bytes(pattern, nbytes, counter=0):
    """what ``dirty`` leaves in an allocation of *nbytes* (the *counter*-th of a block), as a uint8 array"""
    if pattern == "random":
        return np.frombuffer(np.random.default_rng(SEED + counter).bytes(int(nbytes)), np.uint8)
    return np.full(int(nbytes), pattern, np.uint8)


class _Filler:
    def __init__(self, pattern):
        if pattern not in PATTERNS:
            raise ValueError("unknown pattern %r" % (pattern,))
        self.pattern = pattern
        self.count = 0

    def fill(self, device, ptr, nbytes):
        """on the null stream; the caller orders it before the work that follows"""
        n = int(nbytes)
        if n <= 0 or not ptr:
            return
        if self.pattern == "random":
            host = pattern_bytes("random", n, self.count)
            _lib.call("spc_memcpy_h2d", device, C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), n, None)
        else:
            _lib.call("spc_memset", device, C.c_void_p(ptr), int(self.pattern), n, None)
        self.count += 1


@contextlib.contextmanager
def dirty(pattern, device=0):
    """Fill every cached scratch buffer of ``ops.workspace`` with *pattern* now, and every owning ``DeviceArray`` allocation
    (``ptr is None``) made inside the block before its constructor returns - on the class itself, since ops and cube import
    the name.  ``from_numpy`` and ``zeros`` then overwrite their buffers as they do anyway; a scratch buffer that grows inside
    the block is a fresh allocation and is filled like one.  The project's non-blocking streams are not ordered after the
    null stream the fills run on: the device is synchronised after the scratch fills, the null stream after each later one."""
    f = _Filler(pattern)
    with ops._ws_lock:
        cached = list(ops._ws_cache.values())
    for buf in cached:
        f.fill(buf.device, buf.ptr, buf.nbytes)
    original = DeviceArray.__init__

    def init(self, shape, dtype, device=0, ptr=None, owner=None):
        original(self, shape, dtype, device, ptr=ptr, owner=owner)
        if ptr is None and self.nbytes > 0:
            f.fill(self.device, self.ptr, self.nbytes)
            _lib.call("spc_stream_sync", self.device, None)

    DeviceArray.__init__ = init
    try:
        _lib.call("spc_device_sync", device)
        yield f
    finally:
        DeviceArray.__init__ = original


def _differing(got, exp):
    """indices where two arrays of one dtype and shape differ, NaN equal to NaN (test_gpu_views._bits' rule)"""
    return np.argwhere(np.atleast_1d(~((got == exp) | ((got != got) & (exp != exp)))))


def compare(first, later, pattern, first_pattern=PATTERNS[0]):
    """the messages for every output of *later* (run under *pattern*) that is not bit-identical to *first*'s"""
    msgs = []
    if set(first) != set(later):
        return ["pattern %r gives outputs %s, pattern %r gives %s" % (pattern, sorted(later), first_pattern, sorted(first))]
    for name in first:
        a, b = np.asarray(first[name]), np.asarray(later[name])
        if a.dtype != b.dtype or a.shape != b.shape:
            msgs.append("%s under %r: %s %s, under %r: %s %s" % (name, pattern, b.dtype, b.shape, first_pattern, a.dtype, a.shape))
            continue
        bad = _differing(b, a)
        if len(bad):
            at = [tuple(i) if a.ndim else () for i in bad[:4]]
            msgs.append("%s under %r differs from %r at %d places, first %s: %s against %s" % (
                name, pattern, first_pattern, len(bad), [list(map(int, i)) for i in at], [b[i] for i in at], [a[i] for i in at]))
    return msgs


def _as_outputs(r):
    if isinstance(r, dict):
        return r
    if isinstance(r, (tuple, list)):
        return {"out%d" % i: v for i, v in enumerate(r)}
    return {"out": r}


def same_under_every_pattern(run, check=None, patterns=PATTERNS, enter=dirty):
    """``run()`` once per pattern under ``dirty``: every output (a dict of host arrays; a tuple or a single array is named
    out0, out1 ... / out) of every later pattern is bit-identical to the first one's - dtype and shape too, NaN equal to NaN -
    and ``check(first result)`` passes.  The report names the differing patterns, the output, the count and the first
    indices.  Returns the first result."""
    first, failed = None, []
    for p in patterns:
        with enter(p):
            got = _as_outputs(run())
        if first is None:
            first = got
        else:
            failed += compare(first, got, p, patterns[0])
    assert not failed, "the result depends on what memory held:\n" + "\n".join(failed[:12])
    if check is not None:
        check(first)
    return first
