// The 5-point minimal solver of hypotheses5.hip: from five matches to the (at most ten) real essential matrices through them, in
// float64.  include/pats_amd.h ("Per-pair 5-point hypotheses") states the definition; docs/kernels.md 4.10 the design.
//
//   null space  Householder QR of A5^T (9x5, column t = vec(x_r x_l^T) of draw t), as in hypotheses.hip: the last four columns of Q
//               are an orthonormal basis X, Y, Z, W of the null space whatever the rank.  E = x X + y Y + z Z + W
//   cubics      det E = 0 and the nine entries of 2 E E^T E - tr(E E^T) E = 0 as polynomials in (x, y, z): a 10x20 matrix, the
//               columns in Nister's order  x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
//   elimination Gauss-Jordan with partial pivoting on the first ten columns.  Rows 4 .. 9 then read  monomial + (a combination of
//               the last ten) = 0  for x^2z, x^2, y^2z, y^2, xyz, xy;  (row 4) - z (row 5), (6) - z (7), (8) - z (9) are three
//               equations  x p3(z) + y q3(z) + r4(z) = 0:  a 3x3 polynomial matrix whose determinant is a degree-10 polynomial in z
//   roots       a Sturm chain of that polynomial counts the real roots inside the Cauchy bound; root r is bracketed by bisection on
//               the count (at most E5_BISECT steps), then polished by Newton steps on the polynomial that may not leave the bracket
//               (at most E5_NEWTON)
//   models      (x, y, 1) is the null vector of the 3x3 matrix at the root - the largest of the three cross products of its rows, so
//               nothing is divided -, E is normalised, rounded to float32 and CHECKED: a model whose essential residual, evaluated
//               in float64 on the rounded values, exceeds E5_ESS_TOL is dropped, never stored - and so is the second of two
//               roots whose models coincide to E5_DISTINCT (a sample at the edge between k and k + 2 real solutions)
// Every loop has a compile-time trip count.  Everything a lane keeps in registers is indexed statically; what must be indexed
// dynamically (the 10x20 matrix during pivoting) lives in the scratch `S` - LDS on the device, `s(i)` = slot i of this lane.
#pragma once
#include <cstdint>

#ifndef __HIPCC__                                     // a plain host compiler (the solver's stand-alone checks)
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#endif

namespace pats {

constexpr int E5_SLOTS = 200 + 36;                    // the 10x20 matrix, then the null-space basis [4][9]
constexpr int E5_BASIS = 200;
constexpr int E5_MAX_MODELS = 10;
constexpr int E5_BISECT = 64;                         // bisection steps per root, at most
constexpr int E5_NEWTON = 6;                          // Newton steps per root, at most
constexpr double E5_EPS32 = 1.1920928955078125e-07;
constexpr double E5_ESS_TOL = 4.0 * E5_EPS32;         // |2 E E^T E - tr(E E^T) E|_F of a stored model (rounding alone: <= 3 eps32)
constexpr double E5_DISTINCT = 2e-6;                  // a model within 1 - |<a, b>| <= E5_DISTINCT of a stored one of its sample is not stored again
constexpr double E5_ROOT_BOUND = 1e12;                // |z| beyond it is not searched (z^10 stays far inside float64)

#define E5_FN __host__ __device__ __forceinline__
#define E5_UNROLL _Pragma("unroll")

E5_FN double e5_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// ---- monomials of v = (x, y, z, 1): degree 2 as pairs a <= b (10), degree 3 as triples a <= b <= c (20), lexicographic ----------
E5_FN constexpr int e5_idx2(int p, int q) {
    const int a = p < q ? p : q, b = p < q ? q : p;
    return a * 4 - a * (a - 1) / 2 + (b - a);
}
E5_FN constexpr int e5_idx3(int p, int q, int r) {
    const int lo = p < q ? (p < r ? p : r) : (q < r ? q : r), hi = p > q ? (p > r ? p : r) : (q > r ? q : r), mid = p + q + r - lo - hi;
    const int off = lo == 0 ? 0 : (lo == 1 ? 10 : (lo == 2 ? 16 : 19)), k = mid - lo;
    return off + k * (4 - lo) - k * (k - 1) / 2 + (hi - mid);
}
// lexicographic triple -> Nister's column
E5_FN constexpr int e5_col(int n) {
    constexpr int t[20] = {0, 2, 4, 5, 3, 8, 9, 10, 11, 12, 1, 6, 7, 13, 14, 15, 16, 17, 18, 19};
    return t[n];
}

// out (degree 2) += sgn a b, a and b of degree 1
E5_FN void e5_mul11(const double (&a)[4], const double (&b)[4], double sgn, double (&out)[10]) {
    E5_UNROLL
    for (int p = 0; p < 4; ++p) {
        E5_UNROLL
        for (int q = 0; q < 4; ++q) out[e5_idx2(p, q)] = e5_fma(sgn * a[p], b[q], out[e5_idx2(p, q)]);
    }
}
// out (degree 3) += a b, a of degree 2, b of degree 1
E5_FN void e5_mul21(const double (&a)[10], const double (&b)[4], double (&out)[20]) {
    E5_UNROLL
    for (int p = 0; p < 4; ++p) {
        E5_UNROLL
        for (int q = p; q < 4; ++q) {
            E5_UNROLL
            for (int r = 0; r < 4; ++r) out[e5_idx3(p, q, r)] = e5_fma(a[e5_idx2(p, q)], b[r], out[e5_idx3(p, q, r)]);
        }
    }
}

// out[0 .. NA + NB - 2] += sgn a b: polynomials in z, coefficient k at index k
template <int NA, int NB>
E5_FN void e5_pmul(const double (&a)[NA], const double (&b)[NB], double sgn, double (&out)[NA + NB - 1]) {
    E5_UNROLL
    for (int i = 0; i < NA; ++i) {
        E5_UNROLL
        for (int j = 0; j < NB; ++j) out[i + j] = e5_fma(sgn * a[i], b[j], out[i + j]);
    }
}
// the sign changes of the Sturm chain c[k] (degree 10 - k) at z, zeros skipped
E5_FN int e5_changes(const double (&c)[11][11], double z) {
    int n = 0, s = 0;
    E5_UNROLL
    for (int k = 0; k <= 10; ++k) {
        double v = c[k][10 - k];
        E5_UNROLL
        for (int i = 9 - k; i >= 0; --i) v = e5_fma(v, z, c[k][i]);
        const int sg = (v > 0.0) - (v < 0.0);
        if (sg != 0) {
            n += (s != 0 && sg != s) ? 1 : 0;
            s = sg;
        }
    }
    return n;
}

// The solver.  l0 .. r1: the five matches' points (x_l = (l0, l1, 1), x_r = (r0, r1, 1)), finite.  s: this lane's scratch of
// E5_SLOTS doubles.  The models found are written to mo[0 .. 9 count), row-major float32; -> count (0 .. 10)
template <class S>
E5_FN int e5_solve(const double (&l0)[5], const double (&l1)[5], const double (&r0)[5], const double (&r1)[5], S s, float* mo) {
    // ---- the null space: Householder QR of A5^T -----------------------------------------------------------------------------
    {
        double M[9][5], tau[5];
        E5_UNROLL
        for (int t = 0; t < 5; ++t) {
            M[0][t] = r0[t] * l0[t]; M[1][t] = r0[t] * l1[t]; M[2][t] = r0[t];
            M[3][t] = r1[t] * l0[t]; M[4][t] = r1[t] * l1[t]; M[5][t] = r1[t];
            M[6][t] = l0[t];         M[7][t] = l1[t];         M[8][t] = 1.0;
        }
        E5_UNROLL
        for (int k = 0; k < 5; ++k) {
            double ss = 0.0;
            E5_UNROLL
            for (int i = k; i < 9; ++i) ss = e5_fma(M[i][k], M[i][k], ss);
            const double nrm = __builtin_sqrt(ss), x0 = M[k][k];
            const double beta = x0 >= 0.0 ? -nrm : nrm;                                    // x0 - beta never cancels
            const bool live = nrm > 0.0;                                                   // a zero column: H_k = I
            tau[k] = live ? (beta - x0) / beta : 0.0;
            const double inv = live ? 1.0 / (x0 - beta) : 0.0;
            E5_UNROLL
            for (int i = k + 1; i < 9; ++i) M[i][k] *= inv;
            M[k][k] = beta;
            E5_UNROLL
            for (int j = k + 1; j < 5; ++j) {
                double d = M[k][j];
                E5_UNROLL
                for (int i = k + 1; i < 9; ++i) d = e5_fma(M[i][k], M[i][j], d);
                const double w = -(tau[k] * d);
                M[k][j] += w;
                E5_UNROLL
                for (int i = k + 1; i < 9; ++i) M[i][j] = e5_fma(w, M[i][k], M[i][j]);
            }
        }
        E5_UNROLL
        for (int v = 0; v < 4; ++v) {                                                      // Q e_(5 + v) = H_0 .. H_4 e_(5 + v)
            double z[9];
            E5_UNROLL
            for (int i = 0; i < 9; ++i) z[i] = i == 5 + v ? 1.0 : 0.0;
            E5_UNROLL
            for (int k = 4; k >= 0; --k) {
                double d = z[k];
                E5_UNROLL
                for (int i = k + 1; i < 9; ++i) d = e5_fma(M[i][k], z[i], d);
                const double w = -(tau[k] * d);
                z[k] += w;
                E5_UNROLL
                for (int i = k + 1; i < 9; ++i) z[i] = e5_fma(w, M[i][k], z[i]);
            }
            E5_UNROLL
            for (int i = 0; i < 9; ++i) s(E5_BASIS + v * 9 + i) = z[i];
        }
    }
    // ---- the ten cubics ----------------------------------------------------------------------------------------------------
    {
        double Ep[3][3][4];                                                                // entry (i, j) of E as a polynomial in v
        E5_UNROLL
        for (int i = 0; i < 9; ++i) {
            E5_UNROLL
            for (int v = 0; v < 4; ++v) Ep[i / 3][i % 3][v] = s(E5_BASIS + v * 9 + i);
        }
        {                                                                                  // row 0: det E
            double row[20];
            E5_UNROLL
            for (int c = 0; c < 20; ++c) row[c] = 0.0;
            E5_UNROLL
            for (int j = 0; j < 3; ++j) {                                                  // E0j times its cofactor
                const int a = (j + 1) % 3, b = (j + 2) % 3;
                double cof[10];
                E5_UNROLL
                for (int c = 0; c < 10; ++c) cof[c] = 0.0;
                e5_mul11(Ep[1][a], Ep[2][b], 1.0, cof);
                e5_mul11(Ep[1][b], Ep[2][a], -1.0, cof);
                e5_mul21(cof, Ep[0][j], row);
            }
            E5_UNROLL
            for (int c = 0; c < 20; ++c) s(e5_col(c)) = row[c];
        }
        double L[3][3][10];                                                                // 2 E E^T - tr(E E^T) I, symmetric
        E5_UNROLL
        for (int i = 0; i < 3; ++i) {
            E5_UNROLL
            for (int j = i; j < 3; ++j) {
                E5_UNROLL
                for (int c = 0; c < 10; ++c) L[i][j][c] = 0.0;
                E5_UNROLL
                for (int k = 0; k < 3; ++k) e5_mul11(Ep[i][k], Ep[j][k], 1.0, L[i][j]);
            }
        }
        E5_UNROLL
        for (int c = 0; c < 10; ++c) {
            const double tr = L[0][0][c] + L[1][1][c] + L[2][2][c];
            L[0][0][c] = 2.0 * L[0][0][c] - tr; L[1][1][c] = 2.0 * L[1][1][c] - tr; L[2][2][c] = 2.0 * L[2][2][c] - tr;
            L[0][1][c] *= 2.0; L[0][2][c] *= 2.0; L[1][2][c] *= 2.0;
        }
        E5_UNROLL
        for (int i = 0; i < 3; ++i) {
            E5_UNROLL
            for (int j = 0; j < 3; ++j) {                                                  // row 1 + 3 i + j: entry (i, j) of L E
                double row[20];
                E5_UNROLL
                for (int c = 0; c < 20; ++c) row[c] = 0.0;
                E5_UNROLL
                for (int k = 0; k < 3; ++k) e5_mul21(i <= k ? L[i][k] : L[k][i], Ep[k][j], row);
                E5_UNROLL
                for (int c = 0; c < 20; ++c) s((1 + 3 * i + j) * 20 + e5_col(c)) = row[c];
            }
        }
    }
    // ---- Gauss-Jordan with partial pivoting on columns 0 .. 9 -------------------------------------------------------------
    bool ok = true;
    for (int c = 0; c < 10; ++c) {
        int at = c;
        double big = __builtin_fabs(s(c * 20 + c));
        for (int r = c + 1; r < 10; ++r) {
            const double v = __builtin_fabs(s(r * 20 + c));
            if (v > big) { big = v; at = r; }
        }
        double prow[20];
        E5_UNROLL
        for (int j = 0; j < 20; ++j) prow[j] = s(at * 20 + j);
        if (at != c) {
            E5_UNROLL
            for (int j = 0; j < 20; ++j) s(at * 20 + j) = s(c * 20 + j);
        }
        double pv = 0.0;                                                                   // prow[c] without a dynamic register index
        E5_UNROLL
        for (int j = 0; j < 10; ++j) pv = j == c ? prow[j] : pv;
        const double inv = 1.0 / pv;
        ok = ok && pv != 0.0 && __builtin_isfinite(inv);
        E5_UNROLL
        for (int j = 0; j < 20; ++j) {
            prow[j] *= inv;
            s(c * 20 + j) = prow[j];
        }
        for (int r = 0; r < 10; ++r) {
            if (r == c) continue;
            const double f = s(r * 20 + c);
            E5_UNROLL
            for (int j = 0; j < 20; ++j) s(r * 20 + j) = e5_fma(-f, prow[j], s(r * 20 + j));
        }
    }
    // ---- the 3x3 polynomial matrix: row i = (x part [4], y part [4], constant part [5]) in z ------------------------------
    double P[3][13];
    E5_UNROLL
    for (int i = 0; i < 3; ++i) {
        double e[10], f[10];
        E5_UNROLL
        for (int c = 0; c < 10; ++c) {
            e[c] = s((4 + 2 * i) * 20 + 10 + c);
            f[c] = s((5 + 2 * i) * 20 + 10 + c);
        }
        P[i][0] = e[2]; P[i][1] = e[1] - f[2]; P[i][2] = e[0] - f[1]; P[i][3] = -f[0];
        P[i][4] = e[5]; P[i][5] = e[4] - f[5]; P[i][6] = e[3] - f[4]; P[i][7] = -f[3];
        P[i][8] = e[9]; P[i][9] = e[8] - f[9]; P[i][10] = e[7] - f[8]; P[i][11] = e[6] - f[7]; P[i][12] = -f[6];
    }
    double c[11][11];                                                                      // the Sturm chain; c[0] = the determinant
    E5_UNROLL
    for (int k = 0; k < 11; ++k) {
        E5_UNROLL
        for (int i = 0; i < 11; ++i) c[k][i] = 0.0;
    }
    E5_UNROLL
    for (int i = 0; i < 3; ++i) {                                                          // constant part of row i times its cofactor
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        double xa[4], ya[4], xb[4], yb[4], one[5], minor[7];
        E5_UNROLL
        for (int k = 0; k < 4; ++k) { xa[k] = P[a][k]; ya[k] = P[a][4 + k]; xb[k] = P[b][k]; yb[k] = P[b][4 + k]; }
        E5_UNROLL
        for (int k = 0; k < 5; ++k) one[k] = P[i][8 + k];
        E5_UNROLL
        for (int k = 0; k < 7; ++k) minor[k] = 0.0;
        e5_pmul<4, 4>(xa, yb, 1.0, minor);
        e5_pmul<4, 4>(ya, xb, -1.0, minor);
        e5_pmul<7, 5>(minor, one, 1.0, c[0]);
    }
    {
        double top = 0.0;
        E5_UNROLL
        for (int i = 0; i < 11; ++i) top = __builtin_fmax(top, __builtin_fabs(c[0][i]));
        const double inv = 1.0 / top;
        ok = ok && __builtin_isfinite(inv) && __builtin_isfinite(top);
        E5_UNROLL
        for (int i = 0; i < 11; ++i) c[0][i] *= inv;
    }
    ok = ok && c[0][10] != 0.0;
    double bound = 0.0;                                                                    // Cauchy: every root lies in |z| < 1 + max |a_i / a_10|
    E5_UNROLL
    for (int i = 0; i < 10; ++i) bound = __builtin_fmax(bound, __builtin_fabs(c[0][i] / c[0][10]));
    bound = __builtin_fmin(1.0 + bound, E5_ROOT_BOUND);
    ok = ok && bound >= 1.0;                                                               // false for a NaN
    E5_UNROLL
    for (int i = 0; i < 10; ++i) c[1][i] = (double)(i + 1) * c[0][i + 1];
    E5_UNROLL
    for (int k = 1; k < 10; ++k) {                                                         // c[k + 1] = -(c[k - 1] mod c[k]), degrees 10 - k + 1 and 10 - k
        const int d = 10 - k;
        const double lead = c[k][d];
        ok = ok && lead != 0.0 && __builtin_isfinite(lead);
        const double q1 = c[k - 1][d + 1] / lead;
        double a[11];
        a[0] = c[k - 1][0];
        E5_UNROLL
        for (int i = 1; i <= d; ++i) a[i] = e5_fma(-q1, c[k][i - 1], c[k - 1][i]);
        const double q0 = a[d] / lead;
        double top = 0.0;
        E5_UNROLL
        for (int i = 0; i < d; ++i) {
            a[i] = -e5_fma(-q0, c[k][i], a[i]);
            top = __builtin_fmax(top, __builtin_fabs(a[i]));
        }
        const double inv = top > 0.0 ? 1.0 / top : 0.0;                                    // a positive scale: the signs stay
        E5_UNROLL
        for (int i = 0; i < d; ++i) c[k + 1][i] = a[i] * inv;
    }
    if (!ok) return 0;
    const int base = e5_changes(c, -bound);
    const int roots = base - e5_changes(c, bound);                                         // the real roots in (-bound, bound]
    int count = 0;
    for (int r = 0; r < E5_MAX_MODELS; ++r) {
        if (r >= roots) break;
        double lo = -bound, hi = bound;                                                    // roots in (-bound, lo] <= r < roots in (-bound, hi]
        for (int it = 0; it < E5_BISECT; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (!(hi - lo > 1e-10 * __builtin_fmax(1.0, __builtin_fabs(mid)))) break;
            if (base - e5_changes(c, mid) > r) hi = mid; else lo = mid;
        }
        double z = 0.5 * (lo + hi);
        for (int it = 0; it < E5_NEWTON; ++it) {
            double p = c[0][10], dp = 0.0;
            E5_UNROLL
            for (int i = 9; i >= 0; --i) {
                dp = e5_fma(dp, z, p);
                p = e5_fma(p, z, c[0][i]);
            }
            const double zn = z - p / dp;
            if (!(zn >= lo && zn <= hi) || zn == z) break;                                 // also ends on a NaN
            z = zn;
        }
        // (x, y, 1) up to scale: the null vector of the 3x3 matrix at z
        double m[3][3];
        E5_UNROLL
        for (int i = 0; i < 3; ++i) {
            double vx = P[i][3], vy = P[i][7], v1 = P[i][12];
            E5_UNROLL
            for (int k = 2; k >= 0; --k) { vx = e5_fma(vx, z, P[i][k]); vy = e5_fma(vy, z, P[i][4 + k]); }
            E5_UNROLL
            for (int k = 3; k >= 0; --k) v1 = e5_fma(v1, z, P[i][8 + k]);
            m[i][0] = vx; m[i][1] = vy; m[i][2] = v1;
        }
        double w[3] = {0.0, 0.0, 0.0}, wn = -1.0;
        E5_UNROLL
        for (int i = 0; i < 3; ++i) {
            const int a = (i + 1) % 3, b = (i + 2) % 3;
            const double x0 = m[a][1] * m[b][2] - m[a][2] * m[b][1], x1 = m[a][2] * m[b][0] - m[a][0] * m[b][2],
                         x2 = m[a][0] * m[b][1] - m[a][1] * m[b][0];
            const double nn = e5_fma(x0, x0, e5_fma(x1, x1, x2 * x2));
            if (nn > wn) { wn = nn; w[0] = x0; w[1] = x1; w[2] = x2; }
        }
        const double sc = 1.0 / __builtin_sqrt(wn);                                        // keeps the products below in range
        double e[9], nn = 0.0;
        E5_UNROLL
        for (int k = 0; k < 9; ++k) {
            const double zw = e5_fma(z, s(E5_BASIS + 18 + k), s(E5_BASIS + 27 + k));
            e[k] = e5_fma(w[0] * sc, s(E5_BASIS + k), e5_fma(w[1] * sc, s(E5_BASIS + 9 + k), (w[2] * sc) * zw));
            nn = e5_fma(e[k], e[k], nn);
        }
        const double inv = 1.0 / __builtin_sqrt(nn);
        float ef[9];
        double g[9];
        bool good = nn > 0.0;
        E5_UNROLL
        for (int k = 0; k < 9; ++k) {
            ef[k] = (float)(e[k] * inv);
            g[k] = (double)ef[k];
            good = good && __builtin_isfinite(g[k]);
        }
        // the self-check on the values that would be stored: |2 E E^T E - tr(E E^T) E|_F
        double G[3][3], tr = 0.0, res = 0.0;
        E5_UNROLL
        for (int i = 0; i < 3; ++i) {
            E5_UNROLL
            for (int j = 0; j < 3; ++j) G[i][j] = e5_fma(g[3 * i], g[3 * j], e5_fma(g[3 * i + 1], g[3 * j + 1], g[3 * i + 2] * g[3 * j + 2]));
            tr += G[i][i];
        }
        E5_UNROLL
        for (int i = 0; i < 3; ++i) {
            E5_UNROLL
            for (int j = 0; j < 3; ++j) {
                const double v = 2.0 * e5_fma(G[i][0], g[j], e5_fma(G[i][1], g[3 + j], G[i][2] * g[6 + j])) - tr * g[3 * i + j];
                res = e5_fma(v, v, res);
            }
        }
        good = good && __builtin_sqrt(res) <= E5_ESS_TOL && __builtin_fabs(__builtin_sqrt(tr) - 1.0) <= 1e-6;
        if (!good) continue;
        float bigf = __builtin_fabsf(ef[0]), atf = ef[0];                                  // the component of largest magnitude positive
        E5_UNROLL
        for (int k = 1; k < 9; ++k) {
            const float v = __builtin_fabsf(ef[k]);
            if (v > bigf) { bigf = v; atf = ef[k]; }
        }
        const bool flip = atf < 0.0f;
        bool fresh = true;                                                                 // two roots that close give one model
        for (int j = 0; j < E5_MAX_MODELS; ++j) {
            if (j >= count) break;
            double dot = 0.0;
            E5_UNROLL
            for (int k = 0; k < 9; ++k) dot = e5_fma((double)mo[j * 9 + k], g[k], dot);
            fresh = fresh && 1.0 - __builtin_fabs(dot) > E5_DISTINCT;
        }
        if (!fresh) continue;
        E5_UNROLL
        for (int k = 0; k < 9; ++k) mo[count * 9 + k] = flip ? -ef[k] : ef[k];
        ++count;
    }
    return count;
}

}  // namespace pats
