"""What tests/test_awi_host.py and tests/test_gpu_awi.py share: the roundoff bound between two fp64 evaluations of the
adaptive (per-trace matching-filter) misfit (datafit.AdaptiveMatching) that add in different orders and
factor by differently ordered Cholesky algorithms.  Nothing in it comes from the code under test: every quantity is the
twin's, and ||G_j^-1||_2 is NumPy's (eigvalsh of the twin's G_j).

u = 2^-53 is the unit roundoff, U2 = 2 u.  Per trace j, K = 2 L + 1, norms are 2-norms over the K lags.

1. Correlations.  Device and twin form a_j(m) and c_j(k) in fp64 from the same sh, dh as sums of at most nt products, in
   different orders, with or without fma.  As in tests/_traveltime.py each side is off by at most (nt + 1) u times the
   majorant (the same sum of absolute products) to first order, one more u per side stands for the sum over the time
   slices:
       |da(m)| <= (nt + 2) U2 Aa(m),      |dc(k)| <= (nt + 2) U2 Ac(k),      dc := ||(nt + 2) U2 Ac||.
2. The matrix.  G[k, l] = a(|k - l|) + lam a(0) [k == l] is symmetric Toeplitz, so the difference of the two sides' G is
   bounded in the 2-norm by its largest absolute row sum,
       dG_data <= (nt + 2) U2 ((1 + lam) Aa(0) + 2 sum_{m = 1 .. K - 1} Aa(m)) + 2 U2 (1 + lam) a(0),
   the last term for the product lam a(0) and the sum on the diagonal, rounded once each per side (or fused).
3. The solves.  Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 10.4: the solution x^ computed
   by Cholesky factorisation and the two substitutions, in any order of evaluation, satisfies (G + E) x^ = b with
   |E| <= gamma_{3 K + 1} |R^T| |R|, gamma_m = m u / (1 - m u), and || |R^T| |R| ||_2 <= || |R| ||_F^2 = tr(R^T R) = tr(G)
   = K (1 + lam) a(0) (no larger than the K ||G||_2 of his eq. 10.7).  Fused multiply-adds only remove roundings.  Each
   side therefore solves a system whose matrix is off by at most gamma_{3 K + 1} tr(G); against the twin's G, the two
   sides' matrices together are off by
       dG := dG_data + 2 gamma_{3 K + 1} tr(G).
   To first order, with ginv = ||G^-1||_2 of the twin's G:
       ||dw|| <= ginv (dc + dG ||w||) =: ew.
4. W = S / N, S = sum_k t_k^2 w_k^2, N = sum_k w_k^2 has the gradient dW/dw_k = 2 w_k (t_k^2 - W) / N, so
       |dW| <= ||grad W|| ew + (K + 4) U2 W,
   the second term for the evaluation itself: S and N are sums of K non-negative terms (relative error at most
   (K + 2) u each per side whatever the order) and the quotient adds one rounding per side.
5. y_k = tw w_k (t_k^2 - W) / N has the Jacobian (tw / N) (diag(t^2 - W) - w grad W^T - 2 (w . (t^2 - W)) w^T / N); with
   ||grad W|| = 2 ||w . (t^2 - W)|| / N its 2-norm is at most (tw / N) (max_k |t_k^2 - W| + 2 ||w|| ||grad W||) =: Jy, and
       ||dy|| <= Jy ew + 6 U2 ||y||                                       (six roundings per side in the expression)
       ||dz|| <= ginv (||dy|| + dG ||z||) =: ez                           (the second solve, same factor: item 3 again)
6. g[n] = M[n] sum_k z_k dh[n - k] is rows [0, nt) of C z scaled by M, C the (nt + 2 L) x K matrix of the full convolution
   with dh, C^T C = G - mu I, mu = lam a(0).  To first order dz = G^-1 (dy - E z), so M . (C dz) is at most
   max|M| ||C G^-1||_2 (||dy|| + dG ||z||) in norm.  C and G share their right singular vectors: the singular values of
   C G^-1 are sqrt(lambda_i - mu) / lambda_i over the eigenvalues lambda_i of G (NumPy's, as ginv is), at most
   1 / (2 sqrt(mu)); the small eigenvalues of G, which make ginv large, are the directions the convolution damps.
   Adding K terms in another order moves g[n] by at most (K + 2) U2 sum_k |z_k| |dh[n - k]|, in norm at most
   (K + 2) U2 max|M| sqrt(K) ||z|| ||dh||.  With a dtype both sides round g to it once: two roundings of nearly equal
   numbers differ by at most their distance plus one unit of that dtype's round-off (eps) of |g|, which adds
   eps ||g_j||.
Every bound returned is TWICE its first-order value, for the terms of second order.  J = 1/2 sum_j tw_j W_j moves by at
most 1/2 sum_j tw_j bound_W_j, and its own product per term and its sum of ntr terms add (ntr + 2) U2 J."""
import numpy as np

U2 = 2.0 ** -52


class Bounds:
    """per trace: W (s^2), w and z (2-norms over the lags), g (2-norm over time), ginv, cond; J and g_norm (the Frobenius
    norm of the twin's M . g): numbers.  The bounds are 0 for a trace that does not count."""


def roundoff_bounds(obj, d_syn, d_obs, weights=None, trace_weights=None, dtype=None):
    a, c, (Aa, Ac), sh, dh = obj.correlations(d_syn, d_obs, weights)
    nt, ntr = dh.shape
    L, K, lam = obj.L, 2 * obj.L + 1, obj.lam
    tw = obj._trace_weights(trace_weights, ntr)
    G, alive = obj.normal(a)
    F, ok = obj.cholesky(G)
    w = obj.solve(F, c.T)
    t2 = (np.arange(-L, L + 1, dtype=np.float64) * obj.dt) ** 2
    N, S = np.sum(w * w, axis=1), np.sum(t2 * (w * w), axis=1)
    counts = alive & ok & np.isfinite(N) & (N > 0.0)
    Ns = np.where(counts, N, 1.0)
    W = np.where(counts, S / Ns, 0.0)
    y = tw[:, None] * w * (t2[None, :] - W[:, None]) / Ns[:, None]
    z = obj.solve(F, y)
    ev = np.linalg.eigvalsh(G)  # ascending
    ginv, gnorm = 1.0 / ev[:, 0], ev[:, -1]
    u = 0.5 * U2
    gamma = (3 * K + 1) * u / (1.0 - (3 * K + 1) * u)
    dc = np.linalg.norm((nt + 2) * U2 * Ac, axis=0)
    dG = ((nt + 2) * U2 * ((1.0 + lam) * Aa[0] + 2.0 * np.sum(Aa[1:K], axis=0)) + 2.0 * U2 * (1.0 + lam) * a[0]
          + 2.0 * gamma * np.trace(G, axis1=1, axis2=2))
    nrm = lambda x: np.linalg.norm(x, axis=1)  # noqa: E731
    ew = ginv * (dc + dG * nrm(w))
    gradW = 2.0 * nrm(w * (t2[None, :] - W[:, None])) / Ns
    eW = gradW * ew + (K + 4) * U2 * W
    Jy = tw / Ns * (np.max(np.abs(t2[None, :] - W[:, None]), axis=1) + 2.0 * nrm(w) * gradW)
    ey = Jy * ew + 6.0 * U2 * nrm(y)
    ez = ginv * (ey + dG * nrm(z))
    Mmax = 1.0 if weights is None else np.max(np.abs(np.asarray(weights, np.float64)), axis=0)
    dhn = np.linalg.norm(dh, axis=0)
    mu = lam * np.where(alive, a[0], 0.0)
    cginv = np.max(np.sqrt(np.maximum(ev - mu[:, None], 0.0)) / ev, axis=1)  # ||C G^-1||_2
    eg = Mmax * (cginv * (ey + dG * nrm(z)) + np.sqrt(K) * dhn * (K + 2) * U2 * nrm(z))
    b = Bounds()
    b.counts = counts
    b.W = np.where(counts, 2.0 * eW, 0.0)
    b.w = np.where(counts, 2.0 * ew, 0.0)
    b.z = np.where(counts, 2.0 * ez, 0.0)
    b.g = np.where(counts, 2.0 * eg, 0.0)
    g = np.zeros((nt, ntr))  # the twin's M . g before its rounding
    for k in range(-min(L, nt - 1), min(L, nt - 1) + 1):
        if k >= 0:
            g[k:] += z[:, k + L] * dh[:nt - k]
        else:
            g[:nt + k] += z[:, k + L] * dh[-k:]
    g = np.where(counts[None, :], g if weights is None else g * np.asarray(weights, np.float64), 0.0)
    b.g_norm = float(np.linalg.norm(g))
    if dtype is not None:
        b.g = b.g + float(np.finfo(dtype).eps) * np.linalg.norm(g, axis=0)
    b.ginv, b.cond = ginv, gnorm * ginv
    J = float(np.sum(0.5 * tw * W))
    b.J = float(np.sum(0.5 * tw * b.W)) + (ntr + 2) * U2 * J
    return b
