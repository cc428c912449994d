"""Connected components of cube masks on the device: label, sizes, bounding boxes, pruning of small islands.

What users of the reference do on the host with ``scipy.ndimage.label``, ``np.bincount`` and
``scipy.ndimage.find_objects`` on ``cube.get_mask_array()`` (spectral_cube.py:552), here on the uint8 include array where
it lives (ops.label / ops.label_objects / ops.label_select, csrc/spc_label.hip).  :func:`label` returns a :class:`LabelMap`
whose int32 array stays in HBM; its sizes and bounding boxes are two small tables, and ``select`` / :func:`remove_small_objects`
turn a choice of labels back into a :class:`~spectral_cube_amd.masks.DeviceBooleanMask` that goes straight into
``cube.with_mask(...)``.  No cube-sized array travels to the host; scipy itself is never imported.

The labels equal ``scipy.ndimage.label(mask, structure)`` voxel for voxel, numbering included: components are numbered in
raster order of their first voxel.  The structure is 3x3x3 and centrosymmetric (scipy refuses any other), its centre is
ignored, and an all-False structure makes every True voxel a component of its own.  A (3, 3) structure labels every plane
on its own: it becomes the middle plane of a 3x3x3 structure whose other planes are False.

Limits: at most 2**31 - 1 voxels (linear indices are int32; 1024**3 fits); an out-of-core cube is refused (components
cross its strips); cubes sharded over several devices are not labelled; boundaries are not periodic.

``LabelMap.measure(cube)`` and ``LabelMap.catalog(cube)`` measure a cube's samples inside the regions (measurements.py:
the scipy.ndimage measurement family and a flux / peak / centroid / dispersion catalogue, on the device).
"""
import numpy as np

from . import ops
from . import masks as M
from .morphology import _source, generate_binary_structure


def _structure(structure):
    """the (3, 3, 3) bool structure :func:`label` runs with"""
    if structure is None:
        return generate_binary_structure(3, 1)
    s = np.asarray(structure) != 0
    if s.ndim == 2 and s.shape == (3, 3):
        full = np.zeros((3, 3, 3), bool)
        full[1] = s                                   # per plane
        s = full
    if s.shape != (3, 3, 3):
        raise ValueError("structure must have shape (3, 3, 3), or (3, 3) to label every plane on its own (got %s)"
                         % (np.shape(structure),))
    ops.label_structure(s)                            # centrosymmetric, or ValueError
    return s


def pair_bits(structure):
    """the connectivity of *structure* as the kernels read it: bit t = entry t of the (3, 3, 3) structure in C order,
    t < 13 - one bit per pair of opposite neighbours, the centre (entry 13) left out"""
    s = _structure(structure).ravel()
    return int(sum(1 << t for t in range(13) if s[t]))


def keep_table(sizes, bbox, min_size=64, min_channels=1):
    """bool (n + 1,): True for the labels :func:`remove_small_objects` keeps - at least *min_size* voxels and a bounding
    box of at least *min_channels* channels; entry 0 (the background) is False.  Pure numpy on the two host tables."""
    sizes, bbox = np.asarray(sizes), np.asarray(bbox).reshape(-1, 6)
    if sizes.shape[0] != bbox.shape[0]:
        raise ValueError("sizes and bbox must have one entry per label (got %d and %d)" % (sizes.shape[0], bbox.shape[0]))
    keep = (sizes >= min_size) & (bbox[:, 1].astype(np.int64) - bbox[:, 0] >= min_channels) & (sizes > 0)
    keep[:1] = False
    return keep


class LabelMap:
    """The int32 label array of :func:`label` in HBM, with what is asked of it: sizes, bounding boxes, selections."""

    def __init__(self, labels, n, wcs=None):
        self._labels, self.n, self.wcs = labels, int(n), wcs
        self.shape = tuple(labels.shape)
        self._objects = None

    def device_array(self):
        return self._labels

    def get(self):
        """the host int32 array (cube-sized: for inspection)"""
        return self._labels.get()

    def _tables(self):
        if self._objects is None:                     # one ops.label_objects call serves sizes() and find_objects()
            sizes, bbox = ops.label_objects(self._labels, self.n)
            self._objects = (sizes.get(), bbox.get())
        return self._objects

    def sizes(self):
        """host int64 (n + 1,): the voxels of every label, entry 0 the background (np.bincount of the labels)"""
        return self._tables()[0]

    def bounding_boxes(self):
        """host int32 (n + 1, 6): zlo, zhi, ylo, yhi, xlo, xhi of every label, hi exclusive; entry 0 the background"""
        return self._tables()[1]

    def find_objects(self):
        """a list of n tuples of slices, scipy.ndimage.find_objects of the labels (None for a label without a voxel)"""
        sizes, bbox = self._tables()
        return [tuple(slice(int(b[2 * a]), int(b[2 * a + 1]), None) for a in range(3)) if s > 0 else None
                for s, b in zip(sizes[1:], bbox[1:])]

    def select(self, keep):
        """DeviceBooleanMask (the input's WCS): the voxels whose label is kept - *keep*: a bool table of n + 1 entries
        (entry 0: the background), or a list of label numbers.  Only a bool array is a table; a uint8 array, which could be
        either (ops.label_select takes such tables), is refused: pass ``keep.astype(bool)`` or the label numbers as int64"""
        k = np.asarray(keep)
        if k.dtype == np.uint8:
            raise TypeError("a uint8 array could be a keep table or label numbers: pass keep.astype(bool) for a table, "
                            "a list or an int64 array for label numbers")
        if k.dtype != bool:
            numbers = k.astype(np.int64).ravel()
            if numbers.size and (numbers.min() < 0 or numbers.max() > self.n):
                raise ValueError("label numbers must be 0 to %d" % self.n)
            k = np.zeros(self.n + 1, bool)
            k[numbers] = True
        elif k.shape != (self.n + 1,):
            raise ValueError("a keep table has n + 1 = %d entries (got shape %s)" % (self.n + 1, k.shape))
        return M.DeviceBooleanMask(ops.label_select(self._labels, self.n, k), wcs=self.wcs, shape=self.shape)

    def measure(self, cube, want=("sums", "extrema", "first"), origin=None):
        """{table: host array of n + 1 rows}: the samples of *cube* measured inside every label in one pass on the device
        (measurements.measure, ops.label_measure) - count and sums, extrema with their positions, first moments; row 0,
        the background, is never measured.  An out-of-core cube is refused."""
        from . import measurements
        return measurements.measure(cube, self, want=want, origin=origin)

    def catalog(self, cube):
        """a dict of host arrays of length n, one row per label: npix, flux, peak, peak_position, centroid, sigma_z /
        sigma_y / sigma_x, position_angle and, with a WCS, v_cen, sigma_v, lon, lat (measurements.catalog)"""
        from . import measurements
        return measurements.catalog(cube, self)


def label(input, structure=None, cube=None):
    """scipy.ndimage.label of a mask on the device: (LabelMap, n).  *input*: a SpectralCube (its include map), a
    DeviceBooleanMask, any other mask together with *cube* = the cube it is evaluated on (a mask whose lazy terms all
    belong to one cube, ``cube > 3``, finds it itself), or a host bool array of shape (nz, ny, nx).  *structure*: None
    (generate_binary_structure(3, 1)), a centrosymmetric (3, 3, 3) array, or a (3, 3) array that labels every plane on
    its own."""
    s = _structure(structure)
    shape, wcs, owner, fetch = _source(input, cube, "input")
    if owner is not None and owner._stream_source() is not None:
        raise NotImplementedError("labelling needs the whole include map in HBM: an out-of-core cube is refused "
                                  "(components cross its strips)")
    labels, n = ops.label(fetch(cube.device if cube is not None else 0), s)
    return LabelMap(labels, n, wcs), n


def remove_small_objects(input, min_size=64, structure=None, min_channels=1, cube=None):
    """DeviceBooleanMask: *input* (as for :func:`label`) without the components of fewer than *min_size* voxels or whose
    bounding box spans fewer than *min_channels* channels.  Only the two tables (a size and a box per label) travel to
    the host, where :func:`keep_table` decides; the table is uploaded and gathered through the labels on the device."""
    lab, n = label(input, structure=structure, cube=cube)
    return lab.select(keep_table(lab.sizes(), lab.bounding_boxes(), min_size=min_size, min_channels=min_channels))
