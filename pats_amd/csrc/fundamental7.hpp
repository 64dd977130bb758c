// The 7-point minimal solver of hypotheses7.hip: from seven matches to the (at most three) real fundamental matrices through them, in
// float64.  include/pats_amd.h ("Per-pair 7-point hypotheses") states the definition; docs/kernels.md 4.14 the design.
//
//   null space  Householder QR of A7^T (9x7, column t = vec(x_r x_l^T) of draw t), as in essential5.hpp: the last two columns of Q
//               are an orthonormal basis F1, F2 of the null space whatever the rank.  F = a F1 + b F2
//   cubic       det(a F1 + b F2) = c0 a^3 + c1 a^2 b + c2 a b^2 + c3 b^3, a binary cubic: nothing is divided by a leading coefficient,
//               a root at infinity of one chart is the root 0 of the other
//   roots       two charts cover the projective line: x = b / a in [-1, 1] with (a, b) = (1, x), then x = a / b in [-1, 1] with
//               (a, b) = (x, 1) - the same cubic with its coefficients reversed.  In a chart the two critical points of the cubic (one
//               square root) cut [-1, 1] into at most three monotone pieces; a piece whose ends differ in sign holds one root, found
//               by Newton steps that may not leave the bracket and fall back to its midpoint (at most F7_STEPS); an end that is a zero is
//               a root itself
//   models      F = (a F1 + b F2) / |.|, rounded to float32, the component of largest magnitude positive.  A model within F7_DISTINCT
//               of one already stored for the sample is not stored again: a root at x = +-1 belongs to both charts, a double root to
//               two pieces
//   order       the roots of the first chart by ascending b / a, then those of the second by ascending a / b
// Every loop has a compile-time trip count and every index is static once the loops are unrolled: the solver lives in registers.
#pragma once
#include <cstdint>

#ifndef __HIPCC__                                     // a plain host compiler (the solver's stand-alone checks)
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#endif

namespace pats {

constexpr int F7_MAX_MODELS = 3;
constexpr int F7_STEPS = 64;                          // safeguarded Newton steps per root, at most
constexpr double F7_DISTINCT = 2e-6;                  // a model within 1 - |<a, b>| <= F7_DISTINCT of a stored one of its sample is not stored again

#define F7_FN __host__ __device__ __forceinline__
#define F7_UNROLL _Pragma("unroll")

F7_FN double f7_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// k0 + k1 x + k2 x^2 + k3 x^3
F7_FN double f7_eval(const double (&k)[4], double x) { return f7_fma(f7_fma(f7_fma(k[3], x, k[2]), x, k[1]), x, k[0]); }

// x clamped to [-1, 1]; -1 for a NaN
F7_FN double f7_clamp(double x) { return !(x > -1.0) ? -1.0 : (x > 1.0 ? 1.0 : x); }

// the root of the cubic k inside the monotone piece [lo, hi], if there is one
F7_FN bool f7_root(const double (&k)[4], double lo, double hi, double& x) {
    const double flo = f7_eval(k, lo), fhi = f7_eval(k, hi);
    if (flo == 0.0) { x = lo; return true; }
    if (fhi == 0.0) { x = hi; return true; }
    if ((flo < 0.0) == (fhi < 0.0)) return false;
    const bool up = flo < 0.0;                          // the cubic rises over the piece
    x = 0.5 * (lo + hi);
    for (int it = 0; it < F7_STEPS; ++it) {
        double p = k[3], dp = 0.0;
        F7_UNROLL
        for (int i = 2; i >= 0; --i) {
            dp = f7_fma(dp, x, p);
            p = f7_fma(p, x, k[i]);
        }
        if (p == 0.0) break;
        if ((p < 0.0) == up) lo = x; else hi = x;
        double xn = x - p / dp;
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);                                   // also for a NaN
        if (xn == x) break;
        x = xn;
    }
    return true;
}

// the model of (a, b) = (1, x) (chart 0) or (x, 1) (chart 1): normalised, rounded, signed, compared with the `count` models stored
// at mo, and stored behind them if it is new.  -> the new count
F7_FN int f7_store(const double (&F1)[9], const double (&F2)[9], int chart, double x, float* mo, int count) {
    const double a = chart == 0 ? 1.0 : x, b = chart == 0 ? x : 1.0;
    double e[9], nn = 0.0;
    F7_UNROLL
    for (int k = 0; k < 9; ++k) {
        e[k] = f7_fma(a, F1[k], b * F2[k]);
        nn = f7_fma(e[k], e[k], nn);
    }
    const double inv = 1.0 / __builtin_sqrt(nn);
    float ef[9];
    double g[9];
    bool good = nn > 0.0;
    F7_UNROLL
    for (int k = 0; k < 9; ++k) {
        ef[k] = (float)(e[k] * inv);
        g[k] = (double)ef[k];
        good = good && __builtin_isfinite(g[k]);
    }
    if (!good || count >= F7_MAX_MODELS) return count;
    float bigf = __builtin_fabsf(ef[0]), atf = ef[0];                                      // the component of largest magnitude positive
    F7_UNROLL
    for (int k = 1; k < 9; ++k) {
        const float v = __builtin_fabsf(ef[k]);
        if (v > bigf) { bigf = v; atf = ef[k]; }
    }
    const bool flip = atf < 0.0f;
    bool fresh = true;
    for (int j = 0; j < F7_MAX_MODELS; ++j) {
        if (j >= count) break;
        double dot = 0.0;
        F7_UNROLL
        for (int k = 0; k < 9; ++k) dot = f7_fma((double)mo[j * 9 + k], g[k], dot);
        fresh = fresh && 1.0 - __builtin_fabs(dot) > F7_DISTINCT;
    }
    if (!fresh) return count;
    F7_UNROLL
    for (int k = 0; k < 9; ++k) mo[count * 9 + k] = flip ? -ef[k] : ef[k];
    return count + 1;
}

// the roots of chart `chart` (coefficients k) in ascending order, each stored as a model
F7_FN int f7_chart(const double (&k)[4], const double (&F1)[9], const double (&F2)[9], int chart, float* mo, int count) {
    // the critical points: A x^2 + B x + C = 0 without cancellation; a missing one (no real root, A == 0) is clamped to an end
    const double A = 3.0 * k[3], B = 2.0 * k[2], C = k[1];
    const double disc = f7_fma(B, B, -4.0 * A * C);
    double r1 = -1.0, r2 = -1.0;
    if (disc >= 0.0) {
        const double q = -0.5 * (B + (B >= 0.0 ? __builtin_sqrt(disc) : -__builtin_sqrt(disc)));
        r1 = f7_clamp(q / A);
        r2 = f7_clamp(C / q);
        if (r1 > r2) { const double t = r1; r1 = r2; r2 = t; }
    }
    const double cut[4] = {-1.0, r1, r2, 1.0};
    F7_UNROLL
    for (int i = 0; i < 3; ++i) {
        double x;
        if (f7_root(k, cut[i], cut[i + 1], x)) count = f7_store(F1, F2, chart, x, mo, count);
    }
    return count;
}

// The solver.  l0 .. r1: the seven matches' points (x_l = (l0, l1, 1), x_r = (r0, r1, 1)), finite.  The models found are written to
// mo[0 .. 9 count), row-major float32; -> count (0 .. 3)
F7_FN int f7_solve(const double (&l0)[7], const double (&l1)[7], const double (&r0)[7], const double (&r1)[7], float* mo) {
    double F1[9], F2[9];
    // ---- the null space: Householder QR of A7^T --------------------------------------------------------------------------------
    {
        double M[9][7], tau[7];
        F7_UNROLL
        for (int t = 0; t < 7; ++t) {
            M[0][t] = r0[t] * l0[t]; M[1][t] = r0[t] * l1[t]; M[2][t] = r0[t];
            M[3][t] = r1[t] * l0[t]; M[4][t] = r1[t] * l1[t]; M[5][t] = r1[t];
            M[6][t] = l0[t];         M[7][t] = l1[t];         M[8][t] = 1.0;
        }
        F7_UNROLL
        for (int k = 0; k < 7; ++k) {
            double ss = 0.0;
            F7_UNROLL
            for (int i = k; i < 9; ++i) ss = f7_fma(M[i][k], M[i][k], ss);
            const double nrm = __builtin_sqrt(ss), x0 = M[k][k];
            const double beta = x0 >= 0.0 ? -nrm : nrm;                                    // x0 - beta never cancels
            const bool live = nrm > 0.0;                                                   // a zero column: H_k = I
            tau[k] = live ? (beta - x0) / beta : 0.0;
            const double inv = live ? 1.0 / (x0 - beta) : 0.0;
            F7_UNROLL
            for (int i = k + 1; i < 9; ++i) M[i][k] *= inv;
            M[k][k] = beta;
            F7_UNROLL
            for (int j = k + 1; j < 7; ++j) {
                double d = M[k][j];
                F7_UNROLL
                for (int i = k + 1; i < 9; ++i) d = f7_fma(M[i][k], M[i][j], d);
                const double w = -(tau[k] * d);
                M[k][j] += w;
                F7_UNROLL
                for (int i = k + 1; i < 9; ++i) M[i][j] = f7_fma(w, M[i][k], M[i][j]);
            }
        }
        F7_UNROLL
        for (int v = 0; v < 2; ++v) {                                                      // Q e_(7 + v) = H_0 .. H_6 e_(7 + v)
            double z[9];
            F7_UNROLL
            for (int i = 0; i < 9; ++i) z[i] = i == 7 + v ? 1.0 : 0.0;
            F7_UNROLL
            for (int k = 6; k >= 0; --k) {
                double d = z[k];
                F7_UNROLL
                for (int i = k + 1; i < 9; ++i) d = f7_fma(M[i][k], z[i], d);
                const double w = -(tau[k] * d);
                z[k] += w;
                F7_UNROLL
                for (int i = k + 1; i < 9; ++i) z[i] = f7_fma(w, M[i][k], z[i]);
            }
            F7_UNROLL
            for (int i = 0; i < 9; ++i) {
                if (v == 0) F1[i] = z[i]; else F2[i] = z[i];
            }
        }
    }
    // ---- the binary cubic det(a F1 + b F2): entry (i, j) is the form (F1[3 i + j], F2[3 i + j]) ---------------------------------
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    F7_UNROLL
    for (int j = 0; j < 3; ++j) {                                                          // entry (0, j) times its cofactor
        const int u = (j + 1) % 3, v = (j + 2) % 3;
        // cof = (1, u)(2, v) - (1, v)(2, u): a^2, a b, b^2
        const double q0 = f7_fma(F1[3 + u], F1[6 + v], -(F1[3 + v] * F1[6 + u]));
        const double q1 = f7_fma(F1[3 + u], F2[6 + v], F2[3 + u] * F1[6 + v]) - f7_fma(F1[3 + v], F2[6 + u], F2[3 + v] * F1[6 + u]);
        const double q2 = f7_fma(F2[3 + u], F2[6 + v], -(F2[3 + v] * F2[6 + u]));
        c[0] = f7_fma(q0, F1[j], c[0]);
        c[1] = f7_fma(q0, F2[j], f7_fma(q1, F1[j], c[1]));
        c[2] = f7_fma(q1, F2[j], f7_fma(q2, F1[j], c[2]));
        c[3] = f7_fma(q2, F2[j], c[3]);
    }
    double top = 0.0;
    bool ok = true;
    F7_UNROLL
    for (int i = 0; i < 4; ++i) {
        top = __builtin_fmax(top, __builtin_fabs(c[i]));
        ok = ok && __builtin_isfinite(c[i]);
    }
    if (!ok || !(top > 0.0)) return 0;                                                     // an identically vanishing cubic: no model
    const double rev[4] = {c[3], c[2], c[1], c[0]};
    int count = f7_chart(c, F1, F2, 0, mo, 0);
    count = f7_chart(rev, F1, F2, 1, mo, count);
    return count;
}

}  // namespace pats
