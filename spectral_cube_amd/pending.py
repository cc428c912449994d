"""The record of a cube -> cube result that has not been computed yet: the only thing ``SpectralCube._lazy`` holds."""


class Pending:
    """What a producer (``spectral_smooth``, ``reproject``, ``cube + 1``, ...) leaves in the result's ``_lazy`` and what
    the consumers (``_device_data``, ``_strip_plan``, ``_moment_device``, the fused smooth -> moment paths, the
    interpolation ``reproject`` folds in) read.  Every fact a consumer may ask for is a field with a default: a record
    is complete when it is built, a consumer reads fields and never probes, a misspelt keyword raises TypeError here.

    ``record()`` materialises: ``run()`` when given, else ``fn`` on the parent's resident samples and mask (a parent
    above the HBM budget raises HugeCubeError there, which is what a never-resident result is meant to do)."""
    __slots__ = ("fn", "op", "parent", "run", "strips", "slabs", "halo", "keeps_mask", "kernel", "fusable", "arithmetic",
                 "lerp")

    def __init__(self, fn=None, *, op=None, parent=None, run=None, strips=False, slabs=False, halo=0, keeps_mask=False,
                 kernel=None, fusable=False, arithmetic=None, lerp=None):
        if run is None and (fn is None or parent is None):
            raise TypeError("Pending needs run(), or fn(dev, mspec, stream) with the parent cube it reads")
        if (strips or slabs) and (fn is None or parent is None):
            raise TypeError("an out-of-core route needs fn(dev, mspec, stream) and the parent cube")
        self.fn = fn                        # fn(dev, mspec, stream): the operator on the whole cube, a row strip or a slab of planes
        self.op = op                        # operator name ("spectral_smooth", "reproject", ...); None: a plain deferred computation
        self.parent = parent                # the cube whose samples and mask fn reads, or None
        self.run = run                      # run() -> DeviceArray: the resident form, when it is not fn on the parent
        self.strips = bool(strips)          # fn may take row strips (whole spaxels) of an out-of-core parent
        self.slabs = bool(slabs)            # fn may take slabs of whole planes of an out-of-core parent
        self.halo = int(halo)               # rows a strip needs from its neighbours
        self.keeps_mask = bool(keeps_mask)  # the result keeps the parent's mask: the filled form evaluates it on the parent's voxels
        self.kernel = kernel                # taps of a smoothing operator, for a following moment
        self.fusable = bool(fusable)        # a following moment along the spectral axis may run fused with `kernel`
        self.arithmetic = arithmetic        # the arithmetic spatial_smooth was asked for (None: the library's choice)
        self.lerp = lerp                    # (plan, fill) of a pending spectral_interpolate, for a following reproject

    def __call__(self):
        if self.run is not None:
            return self.run()
        return self.fn(self.parent._device_data(), self.parent._mask_spec(), None)
