"""NumPy restatement of the Gaussian smoothing operator (include/fwi.h, fwi_vec_smooth), written from
the definition and kept apart from the package's own forms: per axis of n cells and width sigma,

    R = int(3 sigma + 0.5),  w_k = exp(-k^2 / 2 sigma^2) / sum_j exp(-j^2 / 2 sigma^2),  k = -R .. R,
    (S x)_i = sum_k w_k x_rho(i + k),  rho(j) = -1 - j (j < 0), 2 n - 1 - j (j >= n),

applied x first, then y, then z, in fp64."""
import numpy as np


def radius(sigma):
    return int(3.0 * float(sigma) + 0.5)


def weights(sigma):
    R = radius(sigma)
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) ** 2)) if R else np.ones(1)
    return w / w.sum()


def axis_matrix(n, sigma):
    """The dense n x n matrix of one axis."""
    R = radius(sigma)
    if R > n:
        raise ValueError("R = %d > n = %d" % (R, n))
    w = weights(sigma)
    S = np.zeros((n, n))
    for i in range(n):
        for k in range(-R, R + 1):
            j = i + k
            j = -1 - j if j < 0 else (2 * n - 1 - j if j >= n else j)
            S[i, j] += w[k + R]
    return S


def widths(sigma, ndim):
    s = np.atleast_1d(np.asarray(sigma, np.float64))
    return [float(v) for v in np.broadcast_to(s, (ndim,))]


def gaussian_smooth(x, sigma):
    """S x in fp64 (x is upcast), sigma a scalar or one width per axis."""
    y = np.asarray(x, np.float64)
    for ax, sg in reversed(list(enumerate(widths(sigma, y.ndim)))):
        if radius(sg) == 0:
            continue
        y = np.moveaxis(np.tensordot(axis_matrix(y.shape[ax], sg), y, axes=([1], [ax])), 0, ax)
    return y


def smooth_like(x, sigma):
    """``smooth(x, sigma)`` for ``shots.smoothing_h0``: the restatement, returned in x's dtype."""
    return gaussian_smooth(x, sigma).astype(np.asarray(x).dtype)


def bound(sigma, ndim, u, xmax):
    """Per-cell error bound of one application in a format of unit round-off u: 2 sum_axes (2 R_a + 3) u max|x|
    (a convex combination of 2 R + 1 terms with weights rounded to the format; no pass amplifies; factor 2 margin)."""
    return 2.0 * sum(2 * radius(s) + 3 for s in widths(sigma, ndim) if radius(s) > 0) * u * xmax
