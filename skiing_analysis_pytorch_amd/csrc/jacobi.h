// Cyclic Jacobi of a small symmetric matrix by one thread (essential.hip's nine-vector null space and rotation polish,
// bev.hip's homography).  It is resect.hip's jacobi_lds with one thread doing every lane's part: the same rotations in the
// same order, the same stopping rule and the same zeroing, so tests/resect_restated.py's jacobi restates all three.
#pragma once
#include "fp64_util.h"

namespace skimi {

constexpr int kJacobiSerialSweeps = 60;

// symmetric n x n M (row-major) -> its eigenvalues on M's diagonal, the eigenvectors in the columns of Q
template <int n>
__host__ __device__ inline void jacobi_serial(double* M, double* Q) {
    for (int i = 0; i < n * n; ++i) Q[i] = (i / n == i % n) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSerialSweeps; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int a = 0; a < n; ++a) {
            diag += M[a * n + a] * M[a * n + a];
            for (int b = a + 1; b < n; ++b) off += M[a * n + b] * M[a * n + b];
        }
        if (!is_fin(off) || off <= 1e-40 * diag || off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double mpq = M[p * n + q];
                if (mpq == 0.0) continue;
                const double theta = (M[q * n + q] - M[p * n + p]) / (2.0 * mpq);
                const double tn = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
                for (int k = 0; k < n; ++k) {
                    const double mkp = M[k * n + p], mkq = M[k * n + q];
                    M[k * n + p] = cs * mkp - sn * mkq;
                    M[k * n + q] = sn * mkp + cs * mkq;
                }
                for (int k = 0; k < n; ++k) {
                    const double mpk = M[p * n + k], mqk = M[q * n + k];
                    M[p * n + k] = cs * mpk - sn * mqk;
                    M[q * n + k] = sn * mpk + cs * mqk;
                }
                M[p * n + q] = M[q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double qkp = Q[k * n + p], qkq = Q[k * n + q];
                    Q[k * n + p] = cs * qkp - sn * qkq;
                    Q[k * n + q] = sn * qkp + cs * qkq;
                }
            }
    }
}

}  // namespace skimi
