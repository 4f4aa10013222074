"""What tests/test_transport_host.py and tests/test_gpu_transport.py share: the roundoff bound between two fp64
evaluations of the optimal-transport misfit (datafit.TransportW2) that add in different orders, and the
least distance between a level of F and a level of G, which decides whether two such evaluations take the same indices.

Indices.  m+(n), m-(n) count the levels G_0 .. G_{nt-2} below (or at) the level F_{n-1}, n+(m), n-(m) the other way
round; the clip at nt - 1 leaves the last level of either CDF out.  Two evaluations whose CDFs differ by less than half
the least distance |F_n - G_m| over n, m <= nt - 2 order every pair of levels alike and so get equal index arrays.  A CDF
here is a sum of at most nt positive terms over their total: one evaluation is off by at most (nt + 8) 2^-53 relative
(below), so a least distance of 64 nt 2^-52 (level_gap >= that is what the callers assert) leaves a factor of 32 and more.

The bound.  With equal index arrays the potentials phi, psi are equal integers, formed exactly.  What differs is
f_n = p_n / S_s, g_m = q_m / S_d and the two dual sums of W_j / dt^2 = sum_n phi_n f_n + sum_m psi_m g_m.
  f_n: p_n carries a few ulp of exp, log1p and their sum and quotient (none under the linear transform), S_s is a sum of
  nt positive terms, off by at most (nt - 1) 2^-53 relative whatever the order, and the quotient rounds once: at most
  (nt + 8) 2^-53 relative per evaluation, (nt + 8) 2^-52 between two.  The dual sum moves by at most that times
  sum_n |phi_n| f_n <= max|phi| <= range(phi) = max phi - min phi (phi_0 = 0 lies in the range); likewise for psi.
  the sums: each evaluation rounds every product once (or not at all, by fma) and every partial sum once, at most
  (nt + 1) 2^-53 sum_n |phi_n| f_n, and one more 2^-53 for the sum over the time slices: (nt + 2) 2^-52 between two.
To first order
    |dW_j| <= dt^2 [(nt + 8) 2^-52 (range(phi) + range(psi)) + (nt + 2) 2^-52 (sum_n |phi_n| f_n + sum_m |psi_m| g_m)]
and the bound returned doubles the second factor to (2 nt + 4) 2^-52 for the terms of second order and for the sum of the
two dual sums and the product with dt^2.  Everything is evaluated from the twin's own phi, psi, f, g.
J = 1/2 sum_j w_j W_j then moves by at most sum_j w_j / 2 bound_j, and its own product per term and its sum of ntr terms
add (ntr + 2) 2^-52 J."""
import numpy as np

U2 = 2.0 ** -52


def level_gap(F, G):
    """the least |F_n - G_m| over n, m <= nt - 2 and all traces (inf where nt < 2)"""
    nt, ntr = F.shape
    if nt < 2 or ntr == 0:
        return np.inf
    return float(np.min(np.abs(F[:nt - 1, None, :] - G[None, :nt - 1, :])))


def roundoff_bounds(obj, d_syn, d_obs, weights=None, trace_weights=None):
    """(the bound on |W_j| per trace in s^2, the bound on |J|) from the twin's own potentials and densities; the first is
    0 for a trace that does not count"""
    F, G, f, g, _, _, counts, _, _ = obj.cdfs(d_syn, d_obs, weights)
    nt, ntr = F.shape
    phi, psi = (x.astype(np.float64) for x in obj.potentials(F, G))
    w = np.ones(ntr) if trace_weights is None else np.asarray(trace_weights, np.float64)
    rng = (phi.max(axis=0) - phi.min(axis=0)) + (psi.max(axis=0) - psi.min(axis=0))
    mag = np.sum(np.abs(phi) * f, axis=0) + np.sum(np.abs(psi) * g, axis=0)
    dt2 = obj.dt * obj.dt
    bound = np.where(counts, dt2 * ((nt + 8) * U2 * rng + (2 * nt + 4) * U2 * mag), 0.0)
    W = np.where(counts, dt2 * (np.sum(phi * f, axis=0) + np.sum(psi * g, axis=0)), 0.0)
    J = float(np.sum(0.5 * w * W))
    return bound, float(np.sum(0.5 * w * bound)) + (ntr + 2) * U2 * J
