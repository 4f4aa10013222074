"""NumPy restatement of the regularisers (include/fwi.h, fwi_vec_regularizer), written from the
definition and kept apart from the package's own forms: every axis has its dense n x n forward-difference matrix D_a
(row i: -1 at i, +1 at i + 1; the last row zero), applied along the axis with tensordot, in fp64:

    d = x - x0,  s = sum_a w_a (D_a d)^2,
    tikhonov  R = 1/2 sum s,                      k = 1,
    tv        R = sum (sqrt(s + eps^2) - eps),    k = 1 / sqrt(s + eps^2),
    L(d; v) = sum_a w_a D_a^T (k * (D_a v))."""
import numpy as np


def diff_matrix(n):
    D = np.zeros((n, n))
    for i in range(n - 1):
        D[i, i], D[i, i + 1] = -1.0, 1.0
    return D


def along(M, x, ax):
    """M applied along axis ``ax`` of x."""
    return np.moveaxis(np.tensordot(M, x, axes=([1], [ax])), 0, ax)


def weights(weight, ndim):
    return [float(v) for v in np.broadcast_to(np.atleast_1d(np.asarray(weight, np.float64)), (ndim,))]


def difference(x, x0=None):
    d = np.asarray(x, np.float64)
    return d if x0 is None else d - np.asarray(x0, np.float64)


def s_of(d, w):
    return sum(wa * along(diff_matrix(d.shape[ax]), d, ax) ** 2 for ax, wa in enumerate(w))


def k_of(d, kind, w, eps):
    return np.ones(d.shape) if kind == "tikhonov" else 1.0 / np.sqrt(s_of(d, w) + eps * eps)


def value(x, kind, weight, eps=None, x0=None):
    d = difference(x, x0)
    s = s_of(d, weights(weight, d.ndim))
    return 0.5 * float(np.sum(s)) if kind == "tikhonov" else float(np.sum(np.sqrt(s + eps * eps) - eps))


def apply(x, v, kind, weight, eps=None, x0=None):
    """L(x - x0; v); v = None: v = x - x0."""
    d = difference(x, x0)
    w = weights(weight, d.ndim)
    v = d if v is None else np.asarray(v, np.float64)
    k = k_of(d, kind, w, eps)
    out = np.zeros(d.shape)
    for ax, wa in enumerate(w):
        D = diff_matrix(d.shape[ax])
        out = out + wa * along(D.T, k * along(D, v, ax), ax)
    return out


def majorant(x, v, kind, weight, eps=None, x0=None, alpha=1.0, beta=0.0, out_old=None):
    """M_j = |alpha| sum_a w_a (k_{j-e_a} |D_a v|_{j-e_a} + k_j |D_a v|_j) + |beta| |out_old_j|: the sum of the magnitudes
    of the terms of cell j."""
    d = difference(x, x0)
    w = weights(weight, d.ndim)
    v = d if v is None else np.asarray(v, np.float64)
    k = k_of(d, kind, w, eps)
    M = np.zeros(d.shape)
    for ax, wa in enumerate(w):
        D = diff_matrix(d.shape[ax])
        M = M + wa * along(np.abs(D).T, k * np.abs(along(D, v, ax)), ax)
    M = abs(alpha) * M
    return M if out_old is None or beta == 0.0 else M + abs(beta) * np.abs(np.asarray(out_old, np.float64))
