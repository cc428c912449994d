"""GPU: an error an earlier call left in the runtime's per-thread error state is not reported by the next entry's launch check
as a failed launch of its own (SpcDeviceGuard in spc_common.h reads the state away where every launching entry switches the
device).  The earlier call is one the host tests make too: an entry given a device the machine does not have."""
import ctypes as C

import numpy as np
import pytest

from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu


def test_a_refused_device_switch_does_not_fail_the_next_launch(gpu):
    shape = (8, 4, 16)
    mask = DeviceArray.from_numpy(np.ones(shape, dtype=np.uint8))
    spec = ops.MaskSpec(_lib.MASK_ARRAY, array=mask)
    m = spec.to_c()
    need = int(_lib.load().spc_mask_bits_bytes(*shape))
    bits = DeviceArray((need,), np.uint8)
    with pytest.raises(_lib.HipLibraryError, match="hipSetDevice"):
        _lib.call("spc_mask_pack_bits", 1 << 20, None, shape[0], shape[1], shape[2], C.byref(m), C.c_void_p(bits.ptr), need)
    # the very next launch of this thread, through an entry that checks its launch
    _lib.call("spc_mask_pack_bits", 0, None, shape[0], shape[1], shape[2], C.byref(m), C.c_void_p(bits.ptr), need)
    cube = DeviceArray.from_numpy(np.ones(shape, dtype=np.float32))
    r = ops.moments(cube, DeviceArray.from_numpy(np.arange(8, dtype=np.float64)), mask=spec, want=("m0",))
    assert np.array_equal(r["m0"].get(), np.full(shape[1:], 8.0))
