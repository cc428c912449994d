"""A small stand-in for the ``reproject`` package, written for tools/gen_golden_mosaic.py alone (the package itself is not
available where the golden vectors are made).  It restates, with astropy and scipy, the two functions the reference's
``cube_utils.mosaic_cubes`` / ``combine_headers`` and ``SpectralCube.reproject`` call:

* ``reproject_interp`` - the published steps oracle/oracle_np.py::resample_bilinear already documents: the pixel map from
  ``astropy.wcs`` (target pixel -> sky -> source frame -> source pixel), every channel padded by one edge-replicated
  pixel, ``scipy.ndimage.map_coordinates(padded, coords + 1, order, mode='constant', cval=nan)``, NaN outside
  ``[-0.5, n - 0.5]``, a 3-D footprint.  Only cube headers whose channels coincide are taken (each channel is resampled
  on its own, as oracle_np.reproject_separable does for that case); anything else raises.
* ``mosaicking.find_optimal_celestial_wcs`` - see that module.

Never imported by the package or by a test; only its output (tests/golden/mosaic.npz) is committed.
"""
import numpy as np
from astropy.coordinates import SkyCoord
from astropy.wcs import WCS
from astropy.wcs.utils import wcs_to_celestial_frame
from scipy.ndimage import map_coordinates

ORDERS = {"nearest-neighbor": 0, "bilinear": 1}


def celestial_pixel_map(wcs_in, wcs_out, shape_yx):
    """(xs, ys): 0-based pixel coordinates in *wcs_in* of every pixel of the (ny, nx) grid of *wcs_out*"""
    cin, cout = wcs_in.celestial, wcs_out.celestial
    ny, nx = shape_yx
    yy, xx = np.mgrid[0:ny, 0:nx]
    lon, lat = cout.wcs_pix2world(xx.astype(float), yy.astype(float), 0)
    fin, fout = wcs_to_celestial_frame(cin), wcs_to_celestial_frame(cout)
    sky = SkyCoord(lon, lat, unit="deg", frame=fout).transform_to(fin)
    xs, ys = cin.wcs_world2pix(sky.spherical.lon.deg, sky.spherical.lat.deg, 0)
    return xs, ys


def reproject_interp(input_data, output_projection, shape_out=None, order="bilinear", output_array=None,
                     return_footprint=True, **ignored):
    data, header = input_data
    data = np.asarray(data)
    wcs_in = header if isinstance(header, WCS) else WCS(header)
    wcs_out = output_projection if isinstance(output_projection, WCS) else WCS(output_projection)
    order = ORDERS.get(order, order)
    if order not in (0, 1):
        raise NotImplementedError("the stand-in resamples with order 0 or 1 only")
    nz_out, ny_out, nx_out = (int(n) for n in shape_out)
    nz, ny, nx = data.shape
    z_world = wcs_out.sub([3]).wcs_pix2world(np.arange(nz_out, dtype=float), 0)[0]
    zs = wcs_in.sub([3]).wcs_world2pix(z_world, 0)[0]
    if nz_out != nz or np.abs(zs - np.arange(nz)).max() > 1e-9 * nz:
        raise NotImplementedError("the stand-in takes only targets on the channels of the input")
    xs, ys = celestial_pixel_map(wcs_in, wcs_out, (ny_out, nx_out))
    with np.errstate(invalid="ignore"):
        inside = (xs >= -0.5) & (xs <= nx - 0.5) & (ys >= -0.5) & (ys <= ny - 0.5)
    coords = np.array([np.where(inside, ys, 0.0) + 1.0, np.where(inside, xs, 0.0) + 1.0])
    out = np.empty((nz_out, ny_out, nx_out), dtype=np.float64) if output_array is None else output_array
    for z in range(nz):
        padded = np.pad(np.asarray(data[z], dtype=np.float64), 1, mode="edge")
        plane = map_coordinates(padded, coords, order=order, mode="constant", cval=np.nan)
        plane[~inside] = np.nan
        out[z] = plane
    footprint = np.broadcast_to(inside, out.shape).astype(float)
    return (out, footprint) if return_footprint else out
