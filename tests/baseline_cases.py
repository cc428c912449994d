"""Shared by the baseline tests (test_baseline_host.py, test_gpu_baseline.py): the numpy restatement of the rule stated with
spc_baseline_fit_* / spc_baseline_apply_* in include/spcube_hip.h, the np.linalg.lstsq oracle, the error bound, and the
case table.  Not collected by pytest; importing it touches no GPU.

The restatement loops over the channels of the list and works on whole (ny, nx) maps; numpy rounds every product and every
sum on its own, as the unit built with -ffp-contract=off does, so the device's coefficients, counts and outputs are held
to it bit for bit.  The oracle solves every spectrum by np.linalg.lstsq on the same Legendre design matrix restricted to
the fit set and is compared as model values at all channels, within ``bound``."""
import functools
import itertools

import numpy as np

U = 2.0 ** -53                   # unit roundoff of float64
KAPPA_CAP = 1e6                  # beyond it only npts, the NaN pattern and finiteness are asserted
MAX_ORDER = 5


def abscissa(nz):
    if nz == 1:
        return np.zeros(1)
    return (2.0 * np.arange(nz, dtype=np.float64) - (nz - 1)) / (nz - 1)


def basis(nz, order):
    return np.ascontiguousarray(np.polynomial.legendre.legvander(abscissa(nz), order), dtype=np.float64)


def segment_slices(nfit, nseg):
    """the list positions of every segment: ceil(nfit / nseg) entries each, the last one what is left"""
    n = -(-nfit // nseg)
    return [(i, min(i + n, nfit)) for i in range(0, nfit, n)]


def fit_set(data, include, chan):
    """bool (nz, ny, nx): channel in the list, voxel included, sample not NaN"""
    f = np.zeros(data.shape, bool)
    f[np.asarray(chan, np.int64)] = True
    if include is not None:
        f &= include
    return f & ~np.isnan(data)


def restate_solve(G, b, n, order):
    """c = G^-1 b by G = L D L^T in the header's order, on maps; NaN where n < order + 1 or a pivot is not > 0"""
    m = order + 1
    tri = {}
    for a in range(m):
        for bb in range(a, m):
            tri[a, bb] = len(tri)
    L = [[None] * m for _ in range(m)]
    D = [None] * m
    bad = n < m
    with np.errstate(all="ignore"):
        for j in range(m):
            s = G[tri[j, j]]
            for k in range(j):
                s = s - L[j][k] * (L[j][k] * D[k])
            D[j] = s
            bad = bad | ~(s > 0.0)
            for i in range(j + 1, m):
                r = G[tri[j, i]]
                for k in range(j):
                    r = r - L[i][k] * (L[j][k] * D[k])
                L[i][j] = r / s
        z = [None] * m
        for i in range(m):
            s = b[i]
            for k in range(i):
                s = s - L[i][k] * z[k]
            z[i] = s
        c = [None] * m
        for i in range(m - 1, -1, -1):
            s = z[i] / D[i]
            for k in range(i + 1, m):
                s = s - L[k][i] * c[k]
            c[i] = s
    return np.where(bad[None], np.nan, np.stack(c))


def restate_fit(data, include, chan, order, nseg=1):
    """(coef float64 (order + 1, ny, nx), npts int32 (ny, nx)): the rule of spc_baseline_fit_*; *include*: bool (nz, ny, nx)
    or None; *nseg*: the segment count ops.baseline_segments gives for the shape and len(chan)"""
    nz, ny, nx = data.shape
    m = order + 1
    B = basis(nz, order)
    chan = np.asarray(chan, np.int64)
    pairs = [(a, bb) for a in range(m) for bb in range(a, m)]
    parts = []
    with np.errstate(all="ignore"):
        for i0, i1 in segment_slices(len(chan), nseg):
            G = np.zeros((len(pairs), ny, nx))
            b = np.zeros((m, ny, nx))
            n = np.zeros((ny, nx), np.int32)
            for k in chan[i0:i1]:
                sample = data[k]
                inc = ~np.isnan(sample)
                if include is not None:
                    inc &= include[k]
                dv = sample.astype(np.float64)
                pr = B[k]
                for q, (a, bb) in enumerate(pairs):
                    G[q] = np.where(inc, G[q] + pr[a] * pr[bb], G[q])
                for a in range(m):
                    b[a] = np.where(inc, b[a] + pr[a] * dv, b[a])
                n += inc
            parts.append((G, b, n))
        if len(parts) == 1:
            G, b, n = parts[0]
        else:
            G, b, n = np.zeros_like(parts[0][0]), np.zeros_like(parts[0][1]), np.zeros_like(parts[0][2])
            for pG, pb, pn in parts:
                G, b, n = G + pG, b + pb, n + pn
    return restate_solve(G, b, n, order), n


def restate_apply(data, coef, subtract=True):
    """the rule of spc_baseline_apply_*: model_k = c_0 P[k,0] + c_1 P[k,1] + ... in float64, then v - model or the model"""
    nz = data.shape[0]
    order = coef.shape[0] - 1
    B = basis(nz, order)
    out = np.empty(data.shape, data.dtype)
    with np.errstate(all="ignore"):
        for k in range(nz):
            model = coef[0] * B[k, 0]
            for j in range(1, order + 1):
                model = model + coef[j] * B[k, j]
            out[k] = (data[k].astype(np.float64) - model).astype(data.dtype) if subtract else model.astype(data.dtype)
    return out


def oracle(data, include, chan, order):
    """np.linalg.lstsq per spectrum on the Legendre design matrix restricted to the fit set: dict of ``model`` (float64
    (nz, ny, nx), the fitted values at ALL channels; NaN where n < order + 1), ``coef``, ``npts``, ``kappa`` (kappa_2 of the
    spaxel's Gram matrix) and ``scale`` (max_k sum_j |c_j P_j(t_k)|)"""
    nz, ny, nx = data.shape
    m = order + 1
    B = basis(nz, order)
    f = fit_set(data, include, chan)
    npts = f.sum(axis=0).astype(np.int32)
    model = np.full((nz, ny, nx), np.nan)
    coef = np.full((m, ny, nx), np.nan)
    kappa = np.full((ny, nx), np.nan)
    scale = np.full((ny, nx), np.nan)
    for y in range(ny):
        for x in range(nx):
            if npts[y, x] < m:
                continue
            idx = np.flatnonzero(f[:, y, x])
            A = B[idx]
            c = np.linalg.lstsq(A, data[idx, y, x].astype(np.float64), rcond=None)[0]
            coef[:, y, x] = c
            model[:, y, x] = B @ c
            kappa[y, x] = np.linalg.cond(A.T @ A)
            scale[y, x] = np.abs(B * c[None, :]).sum(axis=1).max()
    return dict(model=model, coef=coef, npts=npts, kappa=kappa, scale=scale)


def bound(n, order, kappa, scale, expected=None, dtype=np.float64):
    """The largest |model - oracle's model| (or, with *expected* = the oracle's output, |output - expected|) the rule allows,
    per spaxel, broadcast over channels.  Nothing here is tuned.

    With m = order + 1, u = 2^-53 and every |P_j(t)| <= 1 on [-1, 1]:

    * sums.  An entry of G or b is a sum of n products, each rounded, added in order: its error is at most
      gamma_(n+1) sum |terms| <= (n + 2) u sum |terms| (Higham, Accuracy and Stability, 3.1).  For G, sum |P_i P_j| <= n =
      G_00 <= ||G||_2, so ||dG||_2 <= ||dG||_F <= m (n + 2) u ||G||_2; b is given the same relative allowance, which makes
      2 m (n + 2) u for the two.
    * solve.  The Cholesky solve of an m-square system is backward stable with ||dG||_2 <= 4 m (3m + 1) u ||G||_2 (Higham,
      10.7); the root-free L D L^T form has the same operation count per entry.
    * conditioning.  ||dc||_2 <= kappa_2(G) (2 m (n + 2) + 4 m (3m + 1)) u ||c||_2 to first order, with kappa_2(G) of that
      spaxel from numpy.
    * scale.  P_j(1) = 1 and t = 1 is the last channel, so s = max_k sum_j |c_j P_j(t_k)| >= ||c||_1 >= ||c||_2; a model
      value moves by at most sum_j |dc_j| <= sqrt(m) ||dc||_2, and its own evaluation, m products and sums, adds (m + 1) u s.
    * output.  float64: one rounding of the difference, u |expected|.  float32: one rounding, 2^-24 (|expected| + b).

    bound = b = (sqrt(m) kappa (2 m (n + 2) + 4 m (3m + 1)) + (m + 1)) u s, plus the output rounding."""
    m = order + 1
    n = np.asarray(n, np.float64)
    b = (np.sqrt(m) * kappa * (2.0 * m * (n + 2.0) + 4.0 * m * (3.0 * m + 1.0)) + (m + 1.0)) * U * scale
    if expected is None:
        return b
    b = np.broadcast_to(b, np.shape(expected))
    mag = np.abs(np.where(np.isfinite(expected), expected, 0.0))
    if np.dtype(dtype) == np.float32:
        return b + 2.0 ** -24 * (mag + b)
    return b + U * mag


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(got, exp):
    """how many elements differ, NaN equal to NaN whatever its payload"""
    got, exp = np.asarray(got), np.asarray(exp)
    return int(np.count_nonzero(~((got == exp) | ((got != got) & (exp != exp)))))


# ---- the case table -------------------------------------------------------------------------------------------------------
PLANES = ((1, 1), (1, 5), (7, 9), (3, 130))
NZS = (1, 2, 7, 37, 64)
MASKS = ("none", "bytes", "finite", "gt")
LISTS = ("all", "ends", "exact")
BYTES = np.array([1, 2, 0x80, 0xFF], np.uint8)           # any non-zero byte includes
GT_THRESHOLD = 0.0
RANDOM_FROM_LISTED = 37                                  # fewer listed channels: random exclusions give rank-deficient or wildly
                                                         # conditioned fit sets, so the exclusions are structured


def channel_list(kind, nz, order):
    if kind == "all":
        return np.arange(nz, dtype=np.int32)
    if kind == "ends":                                   # two end windows of max(nz // 5, order + 1) channels
        w = max(nz // 5, order + 1)
        if 2 * w >= nz:
            return np.arange(nz, dtype=np.int32)
        return np.concatenate([np.arange(w), np.arange(nz - w, nz)]).astype(np.int32)
    if kind == "exact":                                  # exactly order + 1 channels, spread over the band
        return np.unique(np.round(np.linspace(0, nz - 1, order + 1)).astype(np.int32))
    raise KeyError(kind)


def orders_for(nz):
    return tuple(p for p in range(MAX_ORDER + 1) if p + 1 <= nz)


def case_ids():
    """every (plane, nz, order, dtype name, mask, list) of the table"""
    for plane, nz, dt, mask, lst in itertools.product(PLANES, NZS, ("float32", "float64"), MASKS, LISTS):
        for order in orders_for(nz):
            yield plane, nz, order, dt, mask, lst


@functools.lru_cache(maxsize=None)
def make_case(plane, nz, order, dtype, mask, lst):
    """dict of read-only arrays: ``data``; ``mask`` = (kind, uint8 array or None); ``include`` (bool or None: what the mask
    means); ``chan``.  The data are a polynomial of the case's order of size ~10 plus 1 % noise, so that the GT threshold 0
    excludes exactly the voxels pulled below it.  Exclusions: 50 % at random where the list has 37 channels or more, otherwise
    one listed channel per spaxel, entry (y nx + x) mod nfit of the list, while that leaves order + 1.  Planes of three spaxels or more get the special spaxels: spaxel
    0 with n = 0, spaxel 1 with n = order (NaN coefficients) and spaxel 2 with n = order + 1 (finite).  Without a mask an
    exclusion is a NaN sample."""
    ny, nx = plane
    dtype = np.dtype(dtype)
    seed = 1000003 * ny + 10007 * nx + 101 * nz + 13 * order + 7 * MASKS.index(mask) + 3 * LISTS.index(lst) + (dtype.itemsize == 8)
    rng = np.random.default_rng(seed)
    t = abscissa(nz)
    c = rng.uniform(0.5, 1.5, (order + 1, ny, nx)) * np.where(np.arange(order + 1) == 0, 10.0, 1.0)[:, None, None]
    data = np.tensordot(np.polynomial.legendre.legvander(t, order), c, axes=(1, 0))
    data = data + 0.01 * rng.standard_normal(data.shape) + 8.0           # >= 5 - 5 x 1.5 + 8 - noise > 0 everywhere
    chan = channel_list(lst, nz, order)
    listed = np.zeros(nz, bool)
    listed[chan] = True
    if len(chan) >= RANDOM_FROM_LISTED:
        excl = rng.random(data.shape) < 0.5
    else:
        excl = np.zeros(data.shape, bool)
        if len(chan) - 1 >= order + 1:
            k = chan[(np.arange(ny)[:, None] * nx + np.arange(nx)[None, :]) % len(chan)]
            excl[k, np.arange(ny)[:, None], np.arange(nx)[None, :]] = True
    if ny * nx >= 3:
        flat = excl.reshape(nz, ny * nx)
        flat[:, 0] = True
        for spaxel, keep in ((1, order), (2, order + 1)):
            flat[:, spaxel] = True
            pick = chan[np.unique(np.round(np.linspace(0, len(chan) - 1, keep)).astype(int))] if keep else []
            flat[pick, spaxel] = False
    data = data.astype(dtype)
    arr, include = None, None
    if mask == "none":
        data[excl] = np.nan
    elif mask == "bytes":
        arr = np.where(excl, 0, BYTES[rng.integers(0, 4, data.shape)]).astype(np.uint8)
        include = ~excl
    elif mask == "finite":
        data[excl] = np.array([np.nan, np.inf, -np.inf], dtype)[rng.integers(0, 3, int(excl.sum()))]
        include = np.isfinite(data)
    elif mask == "gt":
        data[excl] = -5.0
        include = data > GT_THRESHOLD
    else:
        raise KeyError(mask)
    out = dict(data=data, mask=(mask, arr), include=include, chan=chan, listed=listed)
    for v in (data, arr, include, chan, listed):
        if v is not None:
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_oracle(plane, nz, order, dtype, mask, lst):
    """the oracle of a case, computed once and shared (read-only)"""
    c = make_case(plane, nz, order, dtype, mask, lst)
    o = oracle(c["data"], c["include"], c["chan"], order)
    for v in o.values():
        v.setflags(write=False)
    return o


def toleranced(o, order):
    """bool (ny, nx): the fitted spaxels the toleranced comparison covers (kappa_2(G) <= KAPPA_CAP)"""
    fitted = o["npts"] >= order + 1
    return fitted & (np.where(fitted, o["kappa"], np.inf) <= KAPPA_CAP)
