"""``find_optimal_celestial_wcs`` restated from the documented steps of reproject.mosaicking, with astropy:

the frame is that of the first WCS (or *frame*); every input gives its four outer corners, at 0-based pixels (-0.5, -0.5)
... (nx - 0.5, ny - 0.5), and the sky position of its CRPIX; the reference position is the mean of the CRPIX positions as
unit vectors, normalised (*reference* overrides it); the resolution is the smallest ``proj_plane_pixel_scales`` value of
all inputs (*resolution* overrides it); the target is *projection* with CDELT = (-res, +res), no rotation (``auto_rotate``
is not built) and default LONPOLE / LATPOLE; all corners are projected onto it and CRPIX is shifted so that the smallest
corner coordinate of each axis lies on the outer edge of the first pixel; NAXISn = round(max - min).
"""
import numpy as np
from astropy import units as u
from astropy.coordinates import SkyCoord, UnitSphericalRepresentation
from astropy.wcs.utils import (celestial_frame_to_wcs, pixel_to_skycoord, proj_plane_pixel_scales, skycoord_to_pixel,
                               wcs_to_celestial_frame)


def find_optimal_celestial_wcs(input_data, frame=None, auto_rotate=False, projection="TAN", resolution=None, reference=None):
    if auto_rotate:
        raise NotImplementedError("auto_rotate is not built in the stand-in")
    if frame is None:
        frame = wcs_to_celestial_frame(input_data[0][1])
    corners, references, resolutions = [], [], []
    for shape, wcs in input_data:
        ny, nx = shape
        xc = np.array([-0.5, nx - 0.5, nx - 0.5, -0.5])
        yc = np.array([-0.5, -0.5, ny - 0.5, ny - 0.5])
        corners.append(pixel_to_skycoord(xc, yc, wcs, origin=0).transform_to(frame))
        xp, yp = wcs.wcs.crpix
        references.append(pixel_to_skycoord(xp, yp, wcs, origin=1).transform_to(frame))
        resolutions.append(np.min(proj_plane_pixel_scales(wcs)))
    lon = np.concatenate([c.spherical.lon.deg for c in corners])
    lat = np.concatenate([c.spherical.lat.deg for c in corners])
    if reference is None:
        xyz = np.array([r.represent_as("cartesian").xyz.value / np.linalg.norm(r.represent_as("cartesian").xyz.value)
                        for r in references]).mean(axis=0)
        xyz /= np.linalg.norm(xyz)
        ref_lon = np.degrees(np.arctan2(xyz[1], xyz[0])) % 360.0
        ref_lat = np.degrees(np.arctan2(xyz[2], np.hypot(xyz[0], xyz[1])))
    else:
        if isinstance(reference, SkyCoord):
            reference = reference.transform_to(frame)
            ref_lon, ref_lat = reference.spherical.lon.deg, reference.spherical.lat.deg
        else:
            ref_lon, ref_lat = (float(x) for x in reference)
    if resolution is None:
        resolution = float(np.min(resolutions))
    elif hasattr(resolution, "to"):
        resolution = float(resolution.to(u.deg).value)
    wcs_final = celestial_frame_to_wcs(frame, projection=projection)
    wcs_final.wcs.crval = ref_lon, ref_lat
    wcs_final.wcs.cdelt = -resolution, resolution
    wcs_final.wcs.crpix = 1.0, 1.0
    sky = SkyCoord(UnitSphericalRepresentation(lon * u.deg, lat * u.deg), frame=frame)
    xp, yp = skycoord_to_pixel(sky, wcs_final, origin=1)
    xmin, xmax, ymin, ymax = xp.min(), xp.max(), yp.min(), yp.max()
    wcs_final.wcs.crpix = (1 - xmin) + 0.5, (1 - ymin) + 0.5
    naxis1, naxis2 = int(round(xmax - xmin)), int(round(ymax - ymin))
    return wcs_final, (naxis2, naxis1)
