// The K x K solve of the matching filter's normal equations (fwi_match_solve): plain host C++, no device code and no
// HIP call, so that it builds and runs without a GPU.
//
//   (G + mu I) f = b,   G symmetric (the upper triangle is read), by an fp64 Cholesky factorisation in its
//   square-root-free form G + mu I = L D L^T (L unit lower triangular, D > 0) and forward / back substitution.
//
// No reference counterpart.
#pragma once
#include <cmath>
#include <vector>

namespace fwi {

constexpr int MATCH_SOLVE_KMAX = 129;  // 2 FWI_MATCH_LMAX + 1

// 0: f_out holds the solution.  1: a null argument, K outside [1, MATCH_SOLVE_KMAX], a negative or non-finite mu.
// 2: a pivot that is not positive and finite (the matrix is not positive definite to working precision); f_out is then
// untouched.
inline int match_solve(const double *G, const double *b, int K, double mu, double *f_out) {
    if (!G || !b || !f_out || K < 1 || K > MATCH_SOLVE_KMAX || !(mu >= 0.0) || !std::isfinite(mu)) return 1;
    // G + mu I = L D L^T, L unit lower triangular (kept below the diagonal of Lf), D > 0: the Cholesky factorisation
    // without its square roots, so that K = 1 is the one division b / (G + mu)
    std::vector<double> Lf((size_t)K * K, 0.0), D((size_t)K), y((size_t)K);
    for (int j = 0; j < K; ++j) {
        double dj = G[(size_t)j * K + j] + mu;
        for (int k = 0; k < j; ++k) dj -= Lf[(size_t)j * K + k] * Lf[(size_t)j * K + k] * D[k];
        if (!(dj > 0.0) || !std::isfinite(dj)) return 2;
        D[j] = dj;
        for (int i = j + 1; i < K; ++i) {
            double v = G[(size_t)j * K + i];  // (j, i), j < i: the upper triangle
            for (int k = 0; k < j; ++k) v -= Lf[(size_t)i * K + k] * Lf[(size_t)j * K + k] * D[k];
            Lf[(size_t)i * K + j] = v / dj;
        }
    }
    for (int i = 0; i < K; ++i) {  // L z = b, then y = D^-1 z
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= Lf[(size_t)i * K + k] * y[k];
        y[i] = v;
    }
    for (int i = 0; i < K; ++i) y[i] /= D[i];
    for (int i = K - 1; i >= 0; --i) {  // L^T f = y
        double v = y[i];
        for (int k = i + 1; k < K; ++k) v -= Lf[(size_t)k * K + i] * y[k];
        y[i] = v;
    }
    for (int i = 0; i < K; ++i)
        if (!std::isfinite(y[i])) return 2;
    for (int i = 0; i < K; ++i) f_out[i] = y[i];
    return 0;
}

}  // namespace fwi
