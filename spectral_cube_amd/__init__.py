"""MI355X-native per-spaxel reduction engine for spectral cubes.

Host side: a Python mirror of the reference's SpectralCube operator interface
for the dense hot path (moments, spectral / spatial smoothing, spectral
interpolation, reprojection).  Device side: hand-written HIP kernels for
gfx950 behind the C ABI in include/spcube_hip.h (libspcube_hip.so), bound with
ctypes.  No torch, no CPU fallback.
"""
__version__ = "0.1.0"

from ._lib import HipLibraryError, HipInvalidArgument, HipUnsupported  # noqa: F401
from .cube import (SpectralCube, Projection, VarianceWarning, SmoothingWarning,  # noqa: F401
                   UnitsError, BeamUnitsError, WCSCelestialError, VaryingResolutionSpectralCube, BeamWarning,
                   NonFiniteBeamsWarning, PrecisionWarning, SliceWarning)
from .beam import Beam, BeamError  # noqa: F401
from .masks import (BooleanArrayMask, LazyMask, LazyComparisonMask, CompositeMask,  # noqa: F401
                    FunctionMask, InvertedMask)
from .kernels import (Gaussian1DKernel, Gaussian2DKernel, Box1DKernel, Tophat2DKernel,  # noqa: F401
                      CustomKernel)
from .wcs import SimpleWCS  # noqa: F401
from . import analysis_utilities  # noqa: F401
from .analysis_utilities import stack_spectra, stack_cube, BadVelocitiesWarning  # noqa: F401
from . import cube_utils  # noqa: F401
from .cube_utils import combine_headers, mosaic_cubes  # noqa: F401
from . import morphology  # noqa: F401
from .morphology import (binary_dilation, binary_erosion, binary_opening, binary_closing, binary_propagation,  # noqa: F401
                         generate_binary_structure)
from . import labelling  # noqa: F401
from .labelling import label, remove_small_objects, LabelMap  # noqa: F401
from . import measurements  # noqa: F401
from .measurements import (sum_labels, mean, variance, standard_deviation, minimum, maximum, minimum_position,  # noqa: F401
                           maximum_position, extrema, center_of_mass)
from . import pvextract  # noqa: F401
from .pvextract import Path, extract_pv_slice  # noqa: F401
from . import baseline  # noqa: F401
from .baseline import fit_baseline, subtract_baseline, BaselineFit  # noqa: F401
