// Essential matrix between two calibrated views by RANSAC over five-point hypotheses, and the pose recovered from it
// (cv2.findEssentialMat(RANSAC) + cv2.recoverPose as VideoPose3D/slove_rt_from_3d.py --init essential and
// triangulation/camera_position/camera_position.py call them).  A problem is a group of consecutive correspondences.
//
// Four launches over all groups, no host round trip between them, no allocation, no floating-point atomics:
//   prep_kernel        one workgroup per group: the mask, the used points' ranks in index order (ballot prefix sums) and
//                      their normalised coordinates, compacted into the workspace;
//   hypotheses_kernel  one thread per (group, hypothesis): the counter-based sample and the five-point solver, everything
//                      in the thread's own arrays (9 x 9 Jacobi, the 10 x 20 constraint matrix, Gauss-Jordan, Hessenberg +
//                      Francis QR, null vectors, Gauss-Newton polish): up to ten E per sample into the workspace;
//   score_kernel       the hot loop, one thread per (solution, hypothesis): the group's points staged through LDS in tiles
//                      that every thread of the workgroup reads in rank order (broadcast reads), so a solution's inlier
//                      count and truncated cost are one thread's sums in point order: no reduction, nothing that depends
//                      on the launch shape;
//   finish_kernel      one workgroup per group: the winner by a total order (a strict order, so the tree's shape does not
//                      matter), its inlier mask, the decomposition, the cheirality vote (integer counts), the outputs.
// All arithmetic float64.  The solver's functions are __host__ __device__ so that they can be run on the host against
// tests/essential_restated.py.  Rules: DESIGN §2 "Essential matrix"; include/skimi.h.
#include <math.h>

#include "common.h"
#include "fp64_util.h"
#include "jacobi.h"   // jacobi_serial: the nine-vector null space (rule 4) and the 3 x 3 of the decomposition

namespace skimi {
namespace {

#define HD __host__ __device__ inline

constexpr int kSol = 10;                     // solutions per sample
constexpr int kMinPoints = 5;
constexpr int kPolishSteps = 3;              // DESIGN: the step after which the restatement's iterate is at its rounding floor
constexpr double kResidualBound = 1e-10;     // on max |M mon| / (1 + x^2 + y^2 + z^2)^(3/2) after the polish
constexpr double kPivotTol = 1e-14;
constexpr int kMaxDraws = 64;
constexpr int kMaxHyp = 65536;
constexpr int kTile = 256;                   // points per LDS tile of the scoring loop
constexpr int kScoreThreads = 64;
constexpr int kFinishThreads = 256;

// ---- rule 3: the sampling stream ----------------------------------------------------------------------------------------
HD uint64_t splitmix64(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

HD void draw_sample(uint64_t seed, uint64_t group, uint64_t h, int m, int* sample) {
    uint64_t s = seed ^ ((group << 32) + h);
    splitmix64(s);
    int n = 0;
    for (int outputs = 0; n < 5 && outputs < kMaxDraws; ++outputs) {
        const int r = (int)(splitmix64(s) % (uint64_t)m);
        bool seen = false;
        for (int k = 0; k < n; ++k) seen = seen || sample[k] == r;
        if (!seen) sample[n++] = r;
    }
    for (int r = 0; n < 5; ++r) {
        bool seen = false;
        for (int k = 0; k < n; ++k) seen = seen || sample[k] == r;
        if (!seen) sample[n++] = r;
    }
}

// ---- polynomials in (x, y, z) as homogeneous forms in the variables (x, y, z, 1) = (0, 1, 2, 3): a monomial is a sorted
// index tuple, numbered lexicographically (10 pairs, 20 triples) -----------------------------------------------------------
HD int idx2(int i, int j) {
    if (i > j) { const int t = i; i = j; j = t; }
    return i * 4 - i * (i - 1) / 2 + (j - i);
}
HD int idx3(int i, int j, int k) {
    if (i > j) { const int t = i; i = j; j = t; }
    if (j > k) { const int t = j; j = k; k = t; }
    if (i > j) { const int t = i; i = j; j = t; }
    const int before = i == 0 ? 0 : i == 1 ? 10 : i == 2 ? 16 : 19;
    const int nv = 4 - i, jj = j - i, kk = k - i;
    return before + jj * nv - jj * (jj - 1) / 2 + (kk - jj);
}
// out (degree 2) = p q, both linear
HD void mul11(const double* p, const double* q, double* out) {
    for (int n = 0; n < 10; ++n) out[n] = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out[idx2(i, j)] += p[i] * q[j];
}
// out (degree 3) += sign * p q, p of degree 2, q linear
HD void mul21_acc(const double* p, const double* q, double sign, double* out) {
    double tmp[20];
    for (int n = 0; n < 20; ++n) tmp[n] = 0.0;
    int n = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j, ++n)
            for (int k = 0; k < 4; ++k) tmp[idx3(i, j, k)] += p[n] * q[k];
    for (int m = 0; m < 20; ++m) out[m] += sign * tmp[m];
}

// rule 4's monomial vector and its derivatives at (x, y, z)
HD void monomials(double x, double y, double z, double* mon, double* dx, double* dy, double* dz) {
    const double m[20] = {x * x * x, x * x * y, x * y * y, y * y * y, x * x * z, x * y * z, y * y * z, x * z * z, y * z * z, z * z * z,
                          x * x, x * y, y * y, x * z, y * z, z * z, x, y, z, 1.0};
    for (int k = 0; k < 20; ++k) mon[k] = m[k];
    if (!dx) return;
    const double a[20] = {3 * x * x, 2 * x * y, y * y, 0, 2 * x * z, y * z, 0, z * z, 0, 0, 2 * x, y, 0, z, 0, 0, 1, 0, 0, 0};
    const double b[20] = {0, x * x, 2 * x * y, 3 * y * y, 0, x * z, 2 * y * z, 0, z * z, 0, 0, x, 2 * y, 0, z, 0, 0, 1, 0, 0};
    const double c[20] = {0, 0, 0, 0, x * x, x * y, y * y, 2 * x * z, 2 * y * z, 3 * z * z, 0, 0, 0, x, y, 2 * z, 0, 0, 1, 0};
    for (int k = 0; k < 20; ++k) dx[k] = a[k], dy[k] = b[k], dz[k] = c[k];
}

HD double constraint_residual(const double* M, const double* xyz) {
    double mon[20];
    monomials(xyz[0], xyz[1], xyz[2], mon, nullptr, nullptr, nullptr);
    double worst = 0.0;
    for (int i = 0; i < 10; ++i) {
        double r = 0.0;
        for (int k = 0; k < 20; ++k) r += M[i * 20 + k] * mon[k];
        r = fabs(r);
        if (!(r <= worst)) worst = r;          // keeps a NaN
    }
    const double n2 = 1.0 + (xyz[0] * xyz[0] + xyz[1] * xyz[1] + xyz[2] * xyz[2]);
    return worst / (n2 * sqrt(n2));
}

// one Gauss-Newton step on the ten constraints: d = -(J^T J)^-1 J^T r, LDL^T without pivoting
HD void polish_step(const double* M, double* xyz) {
    double mon[20], dm[3][20];
    monomials(xyz[0], xyz[1], xyz[2], mon, dm[0], dm[1], dm[2]);
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, g[3] = {0, 0, 0};
    for (int i = 0; i < 10; ++i) {
        double r = 0.0, J[3] = {0, 0, 0};
        for (int k = 0; k < 20; ++k) {
            const double c = M[i * 20 + k];
            r += c * mon[k];
            J[0] += c * dm[0][k];
            J[1] += c * dm[1][k];
            J[2] += c * dm[2][k];
        }
        for (int a = 0; a < 3; ++a) {
            g[a] += J[a] * r;
            for (int b = 0; b <= a; ++b) H[a][b] += J[a] * J[b];
        }
    }
    const double d0 = H[0][0];
    const double l10 = H[1][0] / d0, l20 = H[2][0] / d0;
    const double d1 = H[1][1] - l10 * l10 * d0;
    const double l21 = (H[2][1] - l20 * l10 * d0) / d1;
    const double d2 = H[2][2] - l20 * l20 * d0 - l21 * l21 * d1;
    const double y0 = -g[0], y1 = -g[1] - l10 * y0, y2 = -g[2] - l20 * y0 - l21 * y1;
    const double s2 = y2 / d2, s1 = y1 / d1 - l21 * s2, s0 = y0 / d0 - l10 * s1 - l20 * s2;
    xyz[0] += s0, xyz[1] += s1, xyz[2] += s2;
}

// ---- eigenvalues of a general real 10 x 10, after EISPACK's elmhes.f and hqr.f (netlib, public domain; August 1983
// versions, themselves translations of the Algol procedures elmhes and hqr of Martin, Peters and Wilkinson, Handbook for
// Automatic Computation II): stabilised elementary similarity transformations to upper Hessenberg form, then the
// double-shift QR iteration.  The statements follow the Fortran's, its labels turned into loops, low = 1 and igh = n = 10,
// 0-based; its names (en, na, enm2, itn, its, zz, tst1, tst2, notlas) are kept.  false = its error return (no convergence
// within 30 n iterations in all) or a non-finite matrix. -------------------------------------------------------------------
HD double sign_of(double a, double b) { return b >= 0.0 ? fabs(a) : -fabs(a); }      // Fortran's dsign

HD void elmhes(double (*a)[10]) {
    const int n = 10;
    for (int m = 1; m < n - 1; ++m) {
        const int mm1 = m - 1;
        double x = 0.0;
        int i = m;
        for (int j = m; j < n; ++j)
            if (fabs(a[j][mm1]) > fabs(x)) x = a[j][mm1], i = j;
        if (i != m) {                          // interchange rows and columns of a
            for (int j = mm1; j < n; ++j) { const double y = a[i][j]; a[i][j] = a[m][j]; a[m][j] = y; }
            for (int j = 0; j < n; ++j) { const double y = a[j][i]; a[j][i] = a[j][m]; a[j][m] = y; }
        }
        if (x == 0.0) continue;
        for (i = m + 1; i < n; ++i) {
            double y = a[i][mm1];
            if (y == 0.0) continue;
            y = y / x;
            a[i][mm1] = y;
            for (int j = m; j < n; ++j) a[i][j] = a[i][j] - y * a[m][j];
            for (int j = 0; j < n; ++j) a[j][m] = a[j][m] + y * a[j][i];
        }
    }
    for (int i = 2; i < n; ++i)                // the multipliers elmhes leaves below the subdiagonal are not needed
        for (int j = 0; j < i - 1; ++j) a[i][j] = 0.0;
}

HD bool hqr(double (*h)[10], double* wr, double* wi) {
    const int n = 10;
    double norm = 0.0;                         // the norm, used only to judge a zero pair of diagonal entries
    for (int i = 0; i < n; ++i)
        for (int j = (i > 0 ? i - 1 : 0); j < n; ++j) norm = norm + fabs(h[i][j]);
    if (!is_fin(norm)) return false;
    int en = n - 1, itn = 30 * n;
    double t = 0.0;
    while (en >= 0) {                          // search for next eigenvalues
        int its = 0;
        const int na = en - 1, enm2 = na - 1;
        for (;;) {
            // look for single small sub-diagonal element
            int l = en;
            for (; l > 0; --l) {
                double s = fabs(h[l - 1][l - 1]) + fabs(h[l][l]);
                if (s == 0.0) s = norm;
                const double tst1 = s, tst2 = tst1 + fabs(h[l][l - 1]);
                if (tst2 == tst1) break;
            }
            // form shift
            double x = h[en][en];
            if (l == en) {                     // one root found
                wr[en] = x + t;
                wi[en] = 0.0;
                en = na;
                break;
            }
            double y = h[na][na], w = h[en][na] * h[na][en];
            if (l == na) {                     // two roots found
                const double p = (y - x) / 2.0, q = p * p + w;
                double zz = sqrt(fabs(q));
                x = x + t;
                if (q >= 0.0) {                // real pair
                    zz = p + sign_of(zz, p);
                    wr[na] = x + zz;
                    wr[en] = wr[na];
                    if (zz != 0.0) wr[en] = x - w / zz;
                    wi[na] = 0.0;
                    wi[en] = 0.0;
                } else {                       // complex pair
                    wr[na] = x + p;
                    wr[en] = x + p;
                    wi[na] = zz;
                    wi[en] = -zz;
                }
                en = enm2;
                break;
            }
            if (itn == 0) return false;
            if (its == 10 || its == 20) {      // form exceptional shift
                t = t + x;
                for (int i = 0; i <= en; ++i) h[i][i] = h[i][i] - x;
                const double s = fabs(h[en][na]) + fabs(h[na][enm2]);
                x = 0.75 * s;
                y = x;
                w = -0.4375 * s * s;
            }
            its = its + 1;
            itn = itn - 1;
            // look for two consecutive small sub-diagonal elements
            double p = 0.0, q = 0.0, r = 0.0;
            int m = enm2;
            for (; m >= l; --m) {
                const double zz = h[m][m];
                r = x - zz;
                double s = y - zz;
                p = (r * s - w) / h[m + 1][m] + h[m][m + 1];
                q = h[m + 1][m + 1] - zz - r - s;
                r = h[m + 2][m + 1];
                s = fabs(p) + fabs(q) + fabs(r);
                p = p / s;
                q = q / s;
                r = r / s;
                if (m == l) break;
                const double tst1 = fabs(p) * (fabs(h[m - 1][m - 1]) + fabs(zz) + fabs(h[m + 1][m + 1]));
                const double tst2 = tst1 + fabs(h[m][m - 1]) * (fabs(q) + fabs(r));
                if (tst2 == tst1) break;
            }
            for (int i = m + 2; i <= en; ++i) {
                h[i][i - 2] = 0.0;
                if (i != m + 2) h[i][i - 3] = 0.0;
            }
            // double qr step involving rows l to en and columns m to en
            for (int k = m; k <= na; ++k) {
                const bool notlas = k != na;
                if (k != m) {
                    p = h[k][k - 1];
                    q = h[k + 1][k - 1];
                    r = notlas ? h[k + 2][k - 1] : 0.0;
                    x = fabs(p) + fabs(q) + fabs(r);
                    if (x == 0.0) continue;
                    p = p / x;
                    q = q / x;
                    r = r / x;
                }
                const double s = sign_of(sqrt(p * p + q * q + r * r), p);
                if (k != m)
                    h[k][k - 1] = -s * x;
                else if (l != m)
                    h[k][k - 1] = -h[k][k - 1];
                p = p + s;
                x = p / s;
                y = q / s;
                const double zz = r / s;
                q = q / p;
                r = r / p;
                for (int j = k; j <= en; ++j) {               // row modification
                    p = h[k][j] + q * h[k + 1][j];
                    if (notlas) {
                        p = p + r * h[k + 2][j];
                        h[k + 2][j] = h[k + 2][j] - p * zz;
                    }
                    h[k][j] = h[k][j] - p * x;
                    h[k + 1][j] = h[k + 1][j] - p * y;
                }
                const int jmax = en < k + 3 ? en : k + 3;
                for (int i = l; i <= jmax; ++i) {             // column modification
                    p = x * h[i][k] + y * h[i][k + 1];
                    if (notlas) {
                        p = p + zz * h[i][k + 2];
                        h[i][k + 2] = h[i][k + 2] - p * r;
                    }
                    h[i][k] = h[i][k] - p;
                    h[i][k + 1] = h[i][k + 1] - p * q;
                }
            }
        }
    }
    return true;
}

// the null vector of A - lam I by elimination with full pivoting -> (x, y, z) = v6..8 / v9; false if there is none
HD bool null_vector(const double (*A)[10], double lam, double* xyz) {
    const int n = 10;
    double B[10][10];
    int col[10];
    for (int i = 0; i < n; ++i) {
        col[i] = i;
        for (int j = 0; j < n; ++j) B[i][j] = A[i][j] - (i == j ? lam : 0.0);
    }
    for (int s = 0; s < n - 1; ++s) {
        int pi = s, pj = s;
        double best = -1.0;
        for (int i = s; i < n; ++i)
            for (int j = s; j < n; ++j)
                if (fabs(B[i][j]) > best) best = fabs(B[i][j]), pi = i, pj = j;
        if (!(best > 0.0) || !is_fin(best)) return false;
        if (pi != s)
            for (int j = 0; j < n; ++j) { const double t = B[pi][j]; B[pi][j] = B[s][j]; B[s][j] = t; }
        if (pj != s) {
            for (int i = 0; i < n; ++i) { const double t = B[i][pj]; B[i][pj] = B[i][s]; B[i][s] = t; }
            const int t = col[pj]; col[pj] = col[s]; col[s] = t;
        }
        for (int i = s + 1; i < n; ++i) {
            const double f = B[i][s] / B[s][s];
            if (f != 0.0)
                for (int j = s; j < n; ++j) B[i][j] -= f * B[s][j];
        }
    }
    double y[10], v[10];
    y[n - 1] = 1.0;
    for (int i = n - 2; i >= 0; --i) {
        double s = 0.0;
        for (int j = i + 1; j < n; ++j) s += B[i][j] * y[j];
        y[i] = -s / B[i][i];
    }
    for (int i = 0; i < n; ++i) v[col[i]] = y[i];
    if (v[9] == 0.0) return false;
    xyz[0] = v[6] / v[9], xyz[1] = v[7] / v[9], xyz[2] = v[8] / v[9];
    return true;
}

// ---- rule 4: a, b = the five correspondences' normalised coordinates -> up to ten E (row-major, ||E||_F = sqrt 2, by x
// ascending), the rest NaN; returns the count ------------------------------------------------------------------------------
HD int five_point_solve(const double (*a)[2], const double (*b)[2], double* E) {
    for (int k = 0; k < kSol * 9; ++k) E[k] = qnan();
    // nullspace basis
    double AtA[81], Q[81], N[4][9];
    {
        double rows[5][9];
        for (int k = 0; k < 5; ++k) {
            const double ah[3] = {a[k][0], a[k][1], 1.0}, bh[3] = {b[k][0], b[k][1], 1.0};
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) rows[k][3 * i + j] = bh[i] * ah[j];
        }
        for (int i = 0; i < 9; ++i)
            for (int j = 0; j < 9; ++j) {
                double s = 0.0;
                for (int k = 0; k < 5; ++k) s += rows[k][i] * rows[k][j];
                AtA[9 * i + j] = s;
            }
        jacobi_serial<9>(AtA, Q);
        bool taken[9] = {false, false, false, false, false, false, false, false, false};
        for (int k = 0; k < 4; ++k) {
            int best = -1;
            for (int i = 0; i < 9; ++i)
                if (!taken[i] && (best < 0 || AtA[10 * i] < AtA[10 * best])) best = i;
            taken[best] = true;
            for (int i = 0; i < 9; ++i) N[k][i] = Q[9 * i + best];
        }
    }
    // the ten constraints over rule 4's monomials
    double M[200];
    {
        const int perm[20] = {0, 1, 4, 10, 2, 5, 11, 7, 13, 16, 3, 6, 12, 8, 14, 17, 9, 15, 18, 19};
        double e[9][4], eet[6][10], tr[10], row[20], t0[10], t1[10];
        for (int c = 0; c < 9; ++c)
            for (int k = 0; k < 4; ++k) e[c][k] = N[k][c];
        // det E
        for (int k = 0; k < 20; ++k) row[k] = 0.0;
        const int minors[3][5] = {{4, 8, 5, 7, 0}, {3, 8, 5, 6, 1}, {3, 7, 4, 6, 2}};
        for (int c = 0; c < 3; ++c) {
            mul11(e[minors[c][0]], e[minors[c][1]], t0);
            mul11(e[minors[c][2]], e[minors[c][3]], t1);
            for (int k = 0; k < 10; ++k) t0[k] -= t1[k];
            mul21_acc(t0, e[minors[c][4]], c == 1 ? -1.0 : 1.0, row);
        }
        for (int k = 0; k < 20; ++k) M[k] = row[perm[k]];
        // E E^T (its upper triangle) and the trace
        int n = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j, ++n) {
                for (int k = 0; k < 10; ++k) eet[n][k] = 0.0;
                for (int c = 0; c < 3; ++c) {
                    mul11(e[3 * i + c], e[3 * j + c], t0);
                    for (int k = 0; k < 10; ++k) eet[n][k] += t0[k];
                }
            }
        for (int k = 0; k < 10; ++k) tr[k] = eet[0][k] + eet[3][k] + eet[5][k];
        const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                for (int k = 0; k < 20; ++k) row[k] = 0.0;
                for (int c = 0; c < 3; ++c) {
                    for (int k = 0; k < 10; ++k) t0[k] = i == c ? 2.0 * eet[sym[i][c]][k] - tr[k] : 2.0 * eet[sym[i][c]][k];
                    mul21_acc(t0, e[3 * c + j], 1.0, row);
                }
                for (int k = 0; k < 20; ++k) M[20 * (1 + 3 * i + j) + k] = row[perm[k]];
            }
    }
    // B = M[:, :10]^-1 M[:, 10:] by Gauss-Jordan with partial pivoting, then the action matrix
    double A[10][10];
    {
        double G[10][20], colmax[10];
        for (int i = 0; i < 10; ++i)
            for (int k = 0; k < 20; ++k) {
                G[i][k] = M[20 * i + k];
                if (!is_fin(G[i][k])) return 0;
            }
        for (int c = 0; c < 10; ++c) {
            colmax[c] = 0.0;
            for (int i = 0; i < 10; ++i) colmax[c] = fmax(colmax[c], fabs(G[i][c]));
        }
        for (int c = 0; c < 10; ++c) {
            int piv = c;
            for (int i = c + 1; i < 10; ++i)
                if (fabs(G[i][c]) > fabs(G[piv][c])) piv = i;
            if (piv != c)
                for (int k = 0; k < 20; ++k) { const double t = G[piv][k]; G[piv][k] = G[c][k]; G[c][k] = t; }
            const double p = G[c][c];
            if (!is_fin(p) || fabs(p) < kPivotTol * colmax[c]) return 0;
            for (int k = 0; k < 20; ++k) G[c][k] = G[c][k] / p;
            for (int r = 0; r < 10; ++r)
                if (r != c) {
                    const double f = G[r][c];
                    for (int k = 0; k < 20; ++k) G[r][k] = G[r][k] - f * G[c][k];
                }
        }
        const int src[6] = {0, 1, 2, 4, 5, 7};
        for (int i = 0; i < 10; ++i)
            for (int j = 0; j < 10; ++j) {
                A[i][j] = i < 6 ? -G[src[i]][10 + j] : 0.0;
                if (!is_fin(A[i][j])) return 0;
            }
        A[6][0] = A[7][1] = A[8][3] = A[9][6] = 1.0;
    }
    // real eigenvalues -> candidates -> polish -> kept, by x ascending
    double wr[10], wi[10];
    {
        double Hs[10][10];
        for (int i = 0; i < 10; ++i)
            for (int j = 0; j < 10; ++j) Hs[i][j] = A[i][j];
        elmhes(Hs);
        if (!hqr(Hs, wr, wi)) return 0;
    }
    double sol[kSol][3];
    int count = 0;
    for (int k = 0; k < 10; ++k) {
        if (wi[k] != 0.0) continue;
        double xyz[3];
        if (!null_vector(A, wr[k], xyz)) continue;
        for (int it = 0; it < kPolishSteps; ++it) polish_step(M, xyz);
        const double res = constraint_residual(M, xyz);
        if (!is_fin(res) || !(res < kResidualBound)) continue;
        int at = count++;                       // stable insertion by x
        for (; at > 0 && sol[at - 1][0] > xyz[0]; --at)
            for (int c = 0; c < 3; ++c) sol[at][c] = sol[at - 1][c];
        for (int c = 0; c < 3; ++c) sol[at][c] = xyz[c];
    }
    for (int s = 0; s < count; ++s) {
        double e[9], n2 = 0.0;
        for (int c = 0; c < 9; ++c) {
            e[c] = sol[s][0] * N[0][c] + sol[s][1] * N[1][c] + sol[s][2] * N[2][c] + N[3][c];
            n2 += e[c] * e[c];
        }
        const double sc = sqrt(2.0) / sqrt(n2);
        for (int c = 0; c < 9; ++c) E[9 * s + c] = e[c] * sc;
    }
    return count;
}

// ---- rule 5: Sampson error of E on the correspondence (a, b) -------------------------------------------------------------
HD double sampson(const double* E, double a0, double a1, double b0, double b1) {
    const double Ea0 = E[0] * a0 + E[1] * a1 + E[2], Ea1 = E[3] * a0 + E[4] * a1 + E[5], Ea2 = E[6] * a0 + E[7] * a1 + E[8];
    const double Eb0 = E[0] * b0 + E[3] * b1 + E[6], Eb1 = E[1] * b0 + E[4] * b1 + E[7];
    const double num = Ea0 * b0 + Ea1 * b1 + Ea2;
    return num * num / (Ea0 * Ea0 + Ea1 * Ea1 + Eb0 * Eb0 + Eb1 * Eb1);
}

// ---- rule 7: the four pose candidates of E: R [4][9], t [4][3] -----------------------------------------------------------
HD void decompose(const double* E, double (*R)[9], double (*t)[3]) {
    double M[9], Q[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
    jacobi_serial<3>(M, Q);
    int k = 0;
    for (int i = 1; i < 3; ++i)
        if (M[4 * i] < M[4 * k]) k = i;
    const int order[3] = {(k + 1) % 3, (k + 2) % 3, k};
    double V[3][3], U[3][3];                   // V[c] = column c
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 3; ++i) V[c][i] = Q[3 * i + order[c]];
    for (int c = 0; c < 2; ++c) {
        double n2 = 0.0;
        for (int i = 0; i < 3; ++i) {
            U[c][i] = E[3 * i] * V[c][0] + E[3 * i + 1] * V[c][1] + E[3 * i + 2] * V[c][2];
            n2 += U[c][i] * U[c][i];
        }
        const double n = sqrt(n2);
        for (int i = 0; i < 3; ++i) U[c][i] = U[c][i] / n;
    }
    U[2][0] = U[0][1] * U[1][2] - U[0][2] * U[1][1];
    U[2][1] = U[0][2] * U[1][0] - U[0][0] * U[1][2];
    U[2][2] = U[0][0] * U[1][1] - U[0][1] * U[1][0];
    // U W V^T = u2 v1^T - u1 v2^T + u3 v3^T;  U W^T V^T = -u2 v1^T + u1 v2^T + u3 v3^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double w = U[1][i] * V[0][j] - U[0][i] * V[1][j], z = U[2][i] * V[2][j];
            R[0][3 * i + j] = R[1][3 * i + j] = w + z;
            R[2][3 * i + j] = R[3][3 * i + j] = -w + z;
        }
    for (int i = 0; i < 3; ++i) {
        t[0][i] = t[2][i] = U[2][i];
        t[1][i] = t[3][i] = -U[2][i];
    }
}

// rule 8: does the correspondence lie in front of both cameras of (R, t), nearer than dmax
HD bool in_front(const double* R, const double* t, double a0, double a1, double b0, double b1, double dmax) {
    const double p0 = R[0] * a0 + R[1] * a1 + R[2], p1 = R[3] * a0 + R[4] * a1 + R[5], p2 = R[6] * a0 + R[7] * a1 + R[8];
    const double pp = p0 * p0 + p1 * p1 + p2 * p2, pb = p0 * b0 + p1 * b1 + p2, bb = b0 * b0 + b1 * b1 + 1.0;
    const double pt = p0 * t[0] + p1 * t[1] + p2 * t[2], bt = b0 * t[0] + b1 * t[1] + t[2];
    const double det = pp * bb - pb * pb;
    const double z0 = (pb * bt - pt * bb) / det, z1 = (pp * bt - pb * pt) / det;
    return is_fin(z0) && is_fin(z1) && z0 > 0.0 && z1 > 0.0 && z0 < dmax && z1 < dmax;
}

// ---- the workspace --------------------------------------------------------------------------------------------------------
struct Workspace {
    double* ab;          // [N, 4]: a group's used points' (a0, a1, b0, b1) by rank, at its base
    double* E;           // [G, H, 10, 9]
    double* cost;        // [G, H, 10]
    int32_t* idx;        // [N]: point index within the group, by rank
    int32_t* flags;      // [N]: by rank: bit 0 inlier, bits 1..4 the candidates' cheirality
    int32_t* m;          // [G]
    int32_t* count;      // [G, H]
    int32_t* inl;        // [G, H, 10]
};
__host__ inline size_t carve(Workspace& w, void* base, int64_t N, int64_t G, int64_t H) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? (char*)base + off : nullptr;
        off += align_up(bytes, 256);
        return p;
    };
    w.ab = (double*)take(sizeof(double) * 4 * N);
    w.E = (double*)take(sizeof(double) * 90 * G * H);
    w.cost = (double*)take(sizeof(double) * 10 * G * H);
    w.idx = (int32_t*)take(sizeof(int32_t) * N);
    w.flags = (int32_t*)take(sizeof(int32_t) * N);
    w.m = (int32_t*)take(sizeof(int32_t) * G);
    w.count = (int32_t*)take(sizeof(int32_t) * G * H);
    w.inl = (int32_t*)take(sizeof(int32_t) * 10 * G * H);
    return off;
}

struct EssentialArgs {
    const double *x2d, *conf, *K;
    double *R, *t, *E, *cost, *confidence;
    uint8_t *inliers, *pose_mask;
    int32_t *n_used, *n_inliers, *n_pose, *cheirality, *winner, *n_solutions, *success;
    long N, gs, G, group_offset;
    int H;
    uint64_t seed;
    double min_conf, threshold, baseline, dmax;
    Workspace w;
};

// rule 2: tau^2 from the threshold in pixels and both views' focal lengths (K is device memory)
__device__ inline double tau2_of(const EssentialArgs& a) {
    const double tau = a.threshold / ((a.K[0] + a.K[4] + a.K[9] + a.K[13]) / 4.0);
    return tau * tau;
}

// ---- stage 1 ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_kernel(EssentialArgs a) {
    __shared__ int wave_total[4];
    __shared__ int running;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x, base = g * a.gs;
    const double* K0 = a.K;
    const double* K1 = a.K + 9;
    if (tid == 0) running = 0;
    __syncthreads();
    for (long start = 0; start < a.gs; start += 256) {
        const long i = start + tid;
        bool used = false;
        double x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        if (i < a.gs) {
            const long p = base + i;
            x0 = a.x2d[2 * p], y0 = a.x2d[2 * p + 1];
            x1 = a.x2d[2 * (a.N + p)], y1 = a.x2d[2 * (a.N + p) + 1];
            used = is_fin(x0) && is_fin(y0) && is_fin(x1) && is_fin(y1);
            if (a.conf) {
                const double w0 = clamp_conf(a.conf[p]), w1 = clamp_conf(a.conf[a.N + p]);
                used = used && w0 >= a.min_conf && w1 >= a.min_conf;
            }
            a.inliers[p] = 0;
            a.pose_mask[p] = 0;
        }
        const unsigned long long bal = __ballot(used);
        const int before = __popcll(bal & ((1ULL << lane) - 1ULL));
        if (lane == 0) wave_total[wave] = __popcll(bal);
        __syncthreads();
        int rank = running + before;
        for (int w = 0; w < wave; ++w) rank += wave_total[w];
        if (used) {
            const double v0 = (y0 - K0[5]) / K0[4], u0 = (x0 - K0[2] - K0[1] * v0) / K0[0];
            const double v1 = (y1 - K1[5]) / K1[4], u1 = (x1 - K1[2] - K1[1] * v1) / K1[0];
            double* ab = a.w.ab + 4 * (base + rank);
            ab[0] = u0, ab[1] = v0, ab[2] = u1, ab[3] = v1;
            a.w.idx[base + rank] = (int32_t)i;
        }
        __syncthreads();
        if (tid == 0) running += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        __syncthreads();
    }
    if (tid == 0) a.w.m[g] = running;
}

// ---- stage 2 ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hypotheses_kernel(EssentialArgs a) {
    const long gh = (long)blockIdx.x * 64 + threadIdx.x;
    if (gh >= a.G * a.H) return;
    const long g = gh / a.H;
    const int h = (int)(gh % a.H);
    const int m = a.w.m[g];
    if (m < kMinPoints) {
        a.w.count[gh] = 0;
        return;
    }
    int sample[5];
    draw_sample(a.seed, (uint64_t)(g + a.group_offset), (uint64_t)h, m, sample);
    double pa[5][2], pb[5][2];
    for (int k = 0; k < 5; ++k) {
        const double* ab = a.w.ab + 4 * (g * a.gs + sample[k]);
        pa[k][0] = ab[0], pa[k][1] = ab[1], pb[k][0] = ab[2], pb[k][1] = ab[3];
    }
    a.w.count[gh] = five_point_solve(pa, pb, a.w.E + 90 * gh);
}

__global__ __launch_bounds__(64) void five_point_kernel(const double* a, const double* b, long S, double* E, int32_t* counts) {
    const long s = (long)blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    double pa[5][2], pb[5][2];
    for (int k = 0; k < 5; ++k) {
        pa[k][0] = a[10 * s + 2 * k], pa[k][1] = a[10 * s + 2 * k + 1];
        pb[k][0] = b[10 * s + 2 * k], pb[k][1] = b[10 * s + 2 * k + 1];
    }
    counts[s] = five_point_solve(pa, pb, E + 90 * s);
}

// ---- stage 3: blockIdx.x = group, blockIdx.y = a block of (solution, hypothesis) slots.  The slots are taken solution-major
// (slot = s H + h): a sample has 4.6 solutions on average and rarely more than 6, so hypothesis-major waves would idle
// more than half their lanes through the whole point loop; this way the waves of the low solution indices are nearly
// full and those of the high ones nearly empty, and a wave with no solution at all leaves before the loop. ------------------
static_assert(kScoreThreads == 64, "a workgroup of score_kernel is one wave: its early exit is uniform");
__global__ __launch_bounds__(kScoreThreads) void score_kernel(EssentialArgs a) {
    __shared__ double tile[kTile][4];
    const long g = blockIdx.x;
    const int m = a.w.m[g];
    if (m < kMinPoints) return;                // uniform over the workgroup
    const int slot = blockIdx.y * kScoreThreads + threadIdx.x;
    const int s = slot / a.H, h = slot % a.H;
    const bool in_range = s < kSol;
    const bool valid = in_range && s < a.w.count[g * a.H + h];
    const long o = kSol * (g * a.H + h) + s;   // the record and E stay hypothesis-major
    if (__ballot(valid) == 0) {                // the whole wave, which is the whole workgroup
        if (in_range) {
            a.w.inl[o] = -1;
            a.w.cost[o] = qnan();
        }
        return;
    }
    double E[9];
    for (int k = 0; k < 9; ++k) E[k] = valid ? a.w.E[9 * o + k] : 0.0;
    const double* ab = a.w.ab + 4 * g * a.gs;
    const double tau2 = tau2_of(a);
    int inl = 0;
    double cost = 0.0;
    for (int start = 0; start < m; start += kTile) {
        const int n = min(kTile, m - start);
        for (int k = threadIdx.x; k < 4 * n; k += kScoreThreads) (&tile[0][0])[k] = ab[4 * (long)start + k];
        __syncthreads();
        if (valid)
            for (int k = 0; k < n; ++k) {
                const double e2 = sampson(E, tile[k][0], tile[k][1], tile[k][2], tile[k][3]);
                const bool in = is_fin(e2) && e2 <= tau2;
                inl += in ? 1 : 0;
                cost += in ? e2 : tau2;
            }
        __syncthreads();
    }
    if (in_range) {
        a.w.inl[o] = valid ? inl : -1;
        a.w.cost[o] = valid ? cost : qnan();
    }
}

// ---- stage 4 ----------------------------------------------------------------------------------------------------------------
struct Best {
    int inl, slot;
    double cost;
};
__device__ inline bool better(const Best& x, const Best& y) {        // rule 6's total order; slot = 10 h + s
    if (x.inl != y.inl) return x.inl > y.inl;
    if (x.cost < y.cost) return true;
    if (y.cost < x.cost) return false;
    return x.slot < y.slot;                                          // equal costs, and NaN ones (a non-finite tau)
}

__global__ __launch_bounds__(kFinishThreads) void finish_kernel(EssentialArgs a) {
    __shared__ Best best[kFinishThreads];
    __shared__ int isum[kFinishThreads][5];
    __shared__ double sE[9], sR[4][9], st[4][3];
    __shared__ int chosen;
    const int tid = threadIdx.x;
    const long g = blockIdx.x, base = g * a.gs;
    const int m = a.w.m[g];
    const double nan = qnan();
    // the winner and the number of solutions
    Best mine{-1, 0x7fffffff, 0.0};
    int nsol = 0;
    if (m >= kMinPoints) {
        for (int slot = tid; slot < kSol * a.H; slot += kFinishThreads) {
            const int inl = a.w.inl[(long)kSol * g * a.H + slot];
            if (inl < 0) continue;
            ++nsol;
            const Best b{inl, slot, a.w.cost[(long)kSol * g * a.H + slot]};
            if (better(b, mine)) mine = b;
        }
    }
    best[tid] = mine;
    isum[tid][0] = nsol;
    __syncthreads();
    for (int o = kFinishThreads / 2; o > 0; o >>= 1) {
        if (tid < o) {
            if (better(best[tid + o], best[tid])) best[tid] = best[tid + o];
            isum[tid][0] += isum[tid + o][0];
        }
        __syncthreads();
    }
    const Best win = best[0];
    nsol = isum[0][0];
    __syncthreads();
    if (win.inl < 0) {                         // uniform: fewer than 5 used points, or no solution at all
        if (tid == 0) {
            for (int k = 0; k < 9; ++k) a.R[9 * g + k] = a.E[9 * g + k] = nan;
            for (int k = 0; k < 3; ++k) a.t[3 * g + k] = nan;
            for (int k = 0; k < 4; ++k) a.cheirality[4 * g + k] = 0;
            a.cost[g] = a.confidence[g] = nan;
            a.n_used[g] = m;
            a.n_inliers[g] = a.n_pose[g] = a.n_solutions[g] = a.success[g] = 0;
            a.winner[2 * g] = a.winner[2 * g + 1] = -1;
        }
        return;
    }
    if (tid == 0) {
        const double* Ew = a.w.E + 9 * ((long)kSol * g * a.H + win.slot);
        double E[9], R[4][9], t[4][3];
        for (int k = 0; k < 9; ++k) sE[k] = E[k] = Ew[k];
        decompose(E, R, t);
        for (int c = 0; c < 4; ++c) {
            for (int k = 0; k < 9; ++k) sR[c][k] = R[c][k];
            for (int k = 0; k < 3; ++k) st[c][k] = t[c][k];
        }
    }
    __syncthreads();
    // the winner's inliers and the four candidates' votes
    int cnt[5] = {0, 0, 0, 0, 0};
    const double tau2 = tau2_of(a);
    const double* ab = a.w.ab + 4 * base;
    for (int r = tid; r < m; r += kFinishThreads) {
        const double a0 = ab[4 * (long)r], a1 = ab[4 * (long)r + 1], b0 = ab[4 * (long)r + 2], b1 = ab[4 * (long)r + 3];
        const double e2 = sampson(sE, a0, a1, b0, b1);
        int f = 0;
        if (is_fin(e2) && e2 <= tau2) {
            f = 1;
            ++cnt[4];
            for (int c = 0; c < 4; ++c)
                if (in_front(sR[c], st[c], a0, a1, b0, b1, a.dmax)) f |= 2 << c, ++cnt[c];
        }
        a.w.flags[base + r] = f;
    }
    for (int k = 0; k < 5; ++k) isum[tid][k] = cnt[k];
    __syncthreads();
    for (int o = kFinishThreads / 2; o > 0; o >>= 1) {
        if (tid < o)
            for (int k = 0; k < 5; ++k) isum[tid][k] += isum[tid + o][k];
        __syncthreads();
    }
    if (tid == 0) {
        int c = 0;
        for (int k = 1; k < 4; ++k)
            if (isum[0][k] > isum[0][c]) c = k;
        chosen = c;
    }
    __syncthreads();
    const int c = chosen;
    for (int r = tid; r < m; r += kFinishThreads) {          // a thread reads back the flags it wrote itself
        const int f = a.w.flags[base + r];
        const long p = base + a.w.idx[base + r];
        a.inliers[p] = (uint8_t)(f & 1);
        a.pose_mask[p] = (uint8_t)((f >> (1 + c)) & 1);
    }
    if (tid == 0) {
        const double* R = sR[c];
        const double* t = st[c];
        const double tx[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                a.R[9 * g + 3 * i + j] = R[3 * i + j];
                a.E[9 * g + 3 * i + j] = tx[3 * i] * R[j] + tx[3 * i + 1] * R[3 + j] + tx[3 * i + 2] * R[6 + j];
            }
        for (int k = 0; k < 3; ++k) a.t[3 * g + k] = a.baseline * t[k];
        for (int k = 0; k < 4; ++k) a.cheirality[4 * g + k] = isum[0][k];
        const int ninl = isum[0][4];
        a.cost[g] = win.cost;
        a.n_used[g] = m;
        a.n_inliers[g] = ninl;
        a.n_pose[g] = isum[0][c];
        a.n_solutions[g] = nsol;
        a.winner[2 * g] = win.slot / kSol;
        a.winner[2 * g + 1] = win.slot % kSol;
        const double w = (double)ninl / (double)m;
        a.confidence[g] = 1.0 - pow(1.0 - w * w * w * w * w, (double)a.H);
        a.success[g] = ninl >= 5 && isum[0][c] > 0 ? 1 : 0;
    }
}

__host__ inline bool sizes_ok(int64_t n_points, int64_t group_size, int32_t hypotheses) {
    if (n_points < 1 || group_size < 1 || group_size > n_points || n_points % group_size != 0) return false;
    if (group_size > 0x7fffffff / 4 || n_points > (1LL << 40)) return false;
    if (hypotheses < 1 || hypotheses > kMaxHyp) return false;
    const int64_t G = n_points / group_size;
    return G <= 0x7fffffffLL && G * hypotheses <= (1LL << 31) / 64;
}
}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_essential_workspace_bytes(int64_t n_points, int64_t group_size, int32_t hypotheses) {
    if (!sizes_ok(n_points, group_size, hypotheses)) return 0;
    Workspace w;
    return carve(w, nullptr, n_points, n_points / group_size, hypotheses);
}

int skimi_essential_ransac(const double* x2d, const double* conf, const double* K, int64_t n_points, int64_t group_size,
                           double min_conf, double threshold, int32_t hypotheses, uint64_t seed, int64_t group_offset,
                           double baseline, double distance_thresh, double* R, double* t, double* E, uint8_t* inliers,
                           uint8_t* pose_mask, int32_t* n_used, int32_t* n_inliers, int32_t* n_pose, int32_t* cheirality,
                           double* cost, int32_t* winner, int32_t* n_solutions, double* confidence, int32_t* success,
                           void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(x2d && K, "skimi_essential_ransac: NULL input");
    SKIMI_CHECK_ARG(R && t && E && inliers && pose_mask && n_used && n_inliers && n_pose && cheirality && cost && winner &&
                        n_solutions && confidence && success,
                    "skimi_essential_ransac: NULL output");
    SKIMI_CHECK_ARG(hypotheses >= 1 && hypotheses <= kMaxHyp, "skimi_essential_ransac: hypotheses = %d outside 1..%d", hypotheses,
                    kMaxHyp);
    SKIMI_CHECK_ARG(n_points >= 1 && group_size >= 1 && group_size <= n_points && n_points % group_size == 0,
                    "skimi_essential_ransac: group_size = %lld does not divide n_points = %lld", (long long)group_size,
                    (long long)n_points);
    SKIMI_CHECK_ARG(sizes_ok(n_points, group_size, hypotheses), "skimi_essential_ransac: %lld points in groups of %lld with %d hypotheses are too many",
                    (long long)n_points, (long long)group_size, hypotheses);
    SKIMI_CHECK_ARG(threshold > 0.0 && threshold <= 1.79769313486231570815e308, "skimi_essential_ransac: threshold = %g is not a positive number",
                    threshold);
    SKIMI_CHECK_ARG(min_conf == min_conf, "skimi_essential_ransac: min_conf is NaN");
    SKIMI_CHECK_ARG(group_offset >= 0 && group_offset <= (1LL << 31), "skimi_essential_ransac: group_offset = %lld outside 0..2^31",
                    (long long)group_offset);
    SKIMI_CHECK_ARG(baseline == baseline && distance_thresh == distance_thresh, "skimi_essential_ransac: baseline or distance_thresh is NaN");
    EssentialArgs a{};
    const int64_t G = n_points / group_size;
    const size_t need = carve(a.w, ws, n_points, G, hypotheses);
    SKIMI_CHECK_ARG(ws && ws_bytes >= need, "skimi_essential_ransac: workspace of %zu bytes, %zu needed", ws_bytes, need);
    a.x2d = x2d, a.conf = conf, a.K = K;
    a.R = R, a.t = t, a.E = E, a.cost = cost, a.confidence = confidence, a.inliers = inliers, a.pose_mask = pose_mask;
    a.n_used = n_used, a.n_inliers = n_inliers, a.n_pose = n_pose, a.cheirality = cheirality, a.winner = winner;
    a.n_solutions = n_solutions, a.success = success;
    a.N = n_points, a.gs = group_size, a.G = G, a.group_offset = group_offset, a.H = hypotheses, a.seed = seed;
    a.min_conf = min_conf, a.baseline = baseline, a.dmax = distance_thresh;
    a.threshold = threshold;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)G), dim3(256), 0, st, a);
    hipLaunchKernelGGL(hypotheses_kernel, dim3((unsigned)cdiv(G * hypotheses, 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)G, (unsigned)cdiv((int64_t)hypotheses * kSol, kScoreThreads)), dim3(kScoreThreads), 0,
                       st, a);
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)G), dim3(kFinishThreads), 0, st, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_five_point(const double* a, const double* b, int64_t samples, double* E, int32_t* counts, void* stream) {
    SKIMI_CHECK_ARG(a && b && E && counts, "skimi_five_point: NULL input or output");
    SKIMI_CHECK_ARG(samples >= 1 && samples <= (1LL << 31), "skimi_five_point: samples = %lld outside 1..2^31", (long long)samples);
    hipLaunchKernelGGL(five_point_kernel, dim3((unsigned)cdiv(samples, 64)), dim3(64), 0, (hipStream_t)stream, a, b, (long)samples, E,
                       counts);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
