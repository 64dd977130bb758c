// The minimal absolute-pose solver of the depth branch (absolute.hip): three 3-D points X_i and their normalised image points r_i
// -> the up to four (R, t) with r_i ~ R X_i + t.  include/pats_amd.h states the contract ("Per-pair absolute pose from depth");
// docs/kernels.md 4.21 the design.
//
// Formulation: Grunert's (J. A. Grunert, "Das Pothenotische Problem in erweiterter Gestalt nebst ueber seine Anwendungen in der
// Geodaesie", Grunerts Archiv fuer Mathematik und Physik 1, 1841; the form reviewed by Haralick, Lee, Ottenberg and Noelle, "Review and
// analysis of solutions of the three point perspective pose estimation problem", IJCV 13(3), 1994), derived here rather than copied:
//   bearings    f_i = (r_i0, r_i1, 1) / |.|, cos(alpha) = f_1 . f_2, cos(beta) = f_0 . f_2, cos(gamma) = f_0 . f_1
//   sides       a^2 = |X_1 - X_2|^2, b^2 = |X_0 - X_2|^2, c^2 = |X_0 - X_1|^2
//   unknowns    the camera distances s_i with the law of cosines on each side; with u = s_1 / s_0, v = s_2 / s_0 and
//               P(v) = 1 + v^2 - 2 v cos(beta) = b^2 / s_0^2 the difference of two of the three equations is linear in u:
//               u = N(v) / D(v),  N = (a^2 - c^2) P - b^2 (v^2 - 1),  D = 2 b^2 (cos(gamma) - v cos(alpha))
//               and the third becomes the quartic  Q(v) = b^2 (D^2 + N^2 - 2 cos(gamma) N D) - c^2 P D^2  - its coefficients come from
//               polynomial products of these pieces, nothing is expanded by hand
//   roots       the positive real roots of Q, isolated without complex arithmetic: the roots of Q'' (closed form) bracket those of
//               Q', these bracket those of Q; every bracket with a sign change is halved P3P_BISECT times and finished by guarded
//               Newton steps.  A double root (no sign change) is a measure-zero sample and is not reported
//   distances   s_0 = b / sqrt(P(v)), s_1 = u s_0, s_2 = v s_0, all positive; then P3P_POLISH Gauss-Newton steps on the three
//               law-of-cosines equations in (s_0, s_1, s_2) (a step is taken only while it lowers the residual)
//   pose        Y_i = s_i f_i; the orthonormal frames (e_1, e_2, e_3) of the X triangle and (g_1, g_2, g_3) of the Y triangle -
//               e_1 along point 0 -> 1, e_3 the normal, e_2 = e_3 x e_1 - give R = sum g_k e_k^T and t = Y_0 - R X_0
//   kept        a solution is kept iff R and t are finite (also after the rounding to float32), the three depths (R X_i + t)_2 are
//               positive and - THE SELF-CHECK - max_i | (R X_i + t)_{0,1} / (R X_i + t)_2 - r_i |_inf <= P3P_SELF_CHECK, evaluated in
//               float64 on the float64 solution (essential5.hpp drops roots by their residual the same way)
//   order       ascending s_0, the camera distance of the first sample point
// Everything is float64 without contraction.  The code below is plain C++: a host program can include it and run the solver.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define P3P_HD __host__ __device__ __forceinline__
#else
#define P3P_HD inline
#endif

namespace pats {

constexpr double P3P_SELF_CHECK = 1e-8;                // the largest reprojection residual of a kept solution on its own sample
constexpr int P3P_BISECT = 48;                         // halvings of a bracket before the Newton steps
constexpr int P3P_NEWTON = 4;
constexpr int P3P_POLISH = 3;
constexpr double P3P_MAX_RATIO = 1e8;                  // the largest v = s_2 / s_0 looked for

P3P_HD double p3p_eval(const double* c, int deg, double x) {
    double y = c[deg];
    for (int k = deg - 1; k >= 0; --k) y = y * x + c[k];
    return y;
}

// the real roots of the polynomial c (ascending coefficients, degree deg) inside [lo, hi] given the roots of its derivative inside
// (lo, hi), ascending: between two neighbours of {lo, crit..., hi} the polynomial is monotone.  -> their number, ascending in `roots`
P3P_HD int p3p_roots_between(const double* c, int deg, const double* crit, int ncrit, double lo, double hi, double* roots) {
    double d[4];                                        // the derivative, for the Newton steps
    for (int k = 1; k <= deg; ++k) d[k - 1] = c[k] * (double)k;
    int n = 0;
    double x0 = lo, f0 = p3p_eval(c, deg, x0);
    for (int i = 0; i <= ncrit; ++i) {
        const double x1 = i < ncrit ? crit[i] : hi;
        if (!(x1 > x0)) continue;
        const double f1 = p3p_eval(c, deg, x1);
        if (f0 == 0.0) {
            if (n < deg) roots[n++] = x0;
        } else if ((f0 < 0.0) != (f1 < 0.0) && f1 != 0.0) {
            double a = x0, b = x1;                      // f(a) has the sign of f0
#pragma unroll 1
            for (int it = 0; it < P3P_BISECT; ++it) {
                const double m = 0.5 * (a + b), fm = p3p_eval(c, deg, m);
                if ((fm < 0.0) == (f0 < 0.0) && fm != 0.0) a = m; else b = m;
            }
            double x = 0.5 * (a + b);
#pragma unroll 1
            for (int it = 0; it < P3P_NEWTON; ++it) {
                const double fx = p3p_eval(c, deg, x), dx = p3p_eval(d, deg - 1, x);
                const double xn = x - fx / dx;
                if (xn >= a && xn <= b) x = xn;         // false for a NaN: the step is dropped
            }
            if (n < deg) roots[n++] = x;
        }
        x0 = x1; f0 = f1;
    }
    return n;
}

// the positive real roots of the quartic q (ascending coefficients) up to P3P_MAX_RATIO, ascending
P3P_HD int p3p_quartic_roots(const double (&q)[5], double* roots) {
    double c1[4], c2[3];
    for (int k = 1; k <= 4; ++k) c1[k - 1] = q[k] * (double)k;
    for (int k = 1; k <= 3; ++k) c2[k - 1] = c1[k] * (double)k;
    const double lo = 0.0, hi = P3P_MAX_RATIO;
    // Q'' = c2[0] + c2[1] x + c2[2] x^2 in closed form (the stable pair of roots); a vanishing leading term leaves the linear root
    double r2[2];
    int n2 = 0;
    if (c2[2] != 0.0) {
        const double disc = c2[1] * c2[1] - 4.0 * c2[2] * c2[0];
        if (disc > 0.0) {
            const double s = __builtin_sqrt(disc), w = -0.5 * (c2[1] + (c2[1] < 0.0 ? -s : s));
            double xa = w / c2[2], xb = w != 0.0 ? c2[0] / w : xa;
            if (xa > xb) { const double t = xa; xa = xb; xb = t; }
            if (xa > lo && xa < hi) r2[n2++] = xa;
            if (xb > lo && xb < hi && xb > xa) r2[n2++] = xb;
        }
    } else if (c2[1] != 0.0) {
        const double x = -c2[0] / c2[1];
        if (x > lo && x < hi) r2[n2++] = x;
    }
    double r1[3];
    const int n1 = p3p_roots_between(c1, 3, r2, n2, lo, hi, r1);
    double crit[3];
    int nc = 0;
    for (int i = 0; i < n1; ++i)
        if (r1[i] > lo && r1[i] < hi && (nc == 0 || r1[i] > crit[nc - 1])) crit[nc++] = r1[i];
    return p3p_roots_between(q, 4, crit, nc, lo, hi, roots);
}

P3P_HD void p3p_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// the determinant of m with column `col` replaced by v (col < 0: of m itself)
P3P_HD double p3p_det3(const double (&m)[3][3], const double* v, int col) {
    double a[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[i][j] = j == col ? v[i] : m[i][j];
    return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
}

// the frame of a triangle: e1 along 0 -> 1, e3 its normal, e2 = e3 x e1 (columns of F, row-major [3][3]: F[k] = e_{k+1})
P3P_HD void p3p_frame(const double (&p)[3][3], double (&F)[3][3]) {
    double d1[3], d2[3];
    for (int k = 0; k < 3; ++k) { d1[k] = p[1][k] - p[0][k]; d2[k] = p[2][k] - p[0][k]; }
    const double n1 = __builtin_sqrt((d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2]);
    for (int k = 0; k < 3; ++k) F[0][k] = d1[k] / n1;
    double nn[3];
    p3p_cross(F[0], d2, nn);
    const double n3 = __builtin_sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
    for (int k = 0; k < 3; ++k) F[2][k] = nn[k] / n3;
    p3p_cross(F[2], F[0], F[1]);
}

// X[i] = the 3-D points, r[i] = the normalised image points (all finite: the caller checked) -> the number of kept solutions, 0 .. 4;
// Rt[s] = solution s as row-major [R | t] in float64, in the stated order
P3P_HD int p3p_solve(const double (&X)[3][3], const double (&r)[3][2], double (&Rt)[4][12]) {
    double f[3][3];
    for (int i = 0; i < 3; ++i) {
        const double nrm = __builtin_sqrt((r[i][0] * r[i][0] + r[i][1] * r[i][1]) + 1.0);
        f[i][0] = r[i][0] / nrm; f[i][1] = r[i][1] / nrm; f[i][2] = 1.0 / nrm;
    }
    double a2 = 0.0, b2 = 0.0, c2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double da = X[1][k] - X[2][k], db = X[0][k] - X[2][k], dc = X[0][k] - X[1][k];
        a2 += da * da; b2 += db * db; c2 += dc * dc;
    }
    if (!(a2 > 0.0 && b2 > 0.0 && c2 > 0.0)) return 0;  // coincident points (or a NaN)
    const double ca = (f[1][0] * f[2][0] + f[1][1] * f[2][1]) + f[1][2] * f[2][2];
    const double cb = (f[0][0] * f[2][0] + f[0][1] * f[2][1]) + f[0][2] * f[2][2];
    const double cg = (f[0][0] * f[1][0] + f[0][1] * f[1][1]) + f[0][2] * f[1][2];
    // ascending coefficients
    const double P[3] = {1.0, -2.0 * cb, 1.0};
    const double N[3] = {(a2 - c2) * P[0] + b2, (a2 - c2) * P[1], (a2 - c2) * P[2] - b2};
    const double D[2] = {2.0 * b2 * cg, -2.0 * b2 * ca};
    double DD[3] = {D[0] * D[0], 2.0 * D[0] * D[1], D[1] * D[1]};
    double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) q[i + j] += b2 * (N[i] * N[j]) - c2 * (P[i] * DD[j]);
    for (int i = 0; i < 3; ++i) q[i] += b2 * DD[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 2; ++j) q[i + j] -= (2.0 * b2 * cg) * (N[i] * D[j]);
    double big = 0.0;
    for (int k = 0; k < 5; ++k) big = __builtin_fabs(q[k]) > big ? __builtin_fabs(q[k]) : big;
    if (!(big > 0.0) || !__builtin_isfinite(big)) return 0;
    for (int k = 0; k < 5; ++k) q[k] /= big;
    double roots[4];
    const int nr = p3p_quartic_roots(q, roots);

    int n = 0;
    double s0s[4];
    for (int ir = 0; ir < nr; ++ir) {
        const double v = roots[ir];
        const double u = p3p_eval(N, 2, v) / p3p_eval(D, 1, v);
        const double s0 = __builtin_sqrt(b2 / p3p_eval(P, 2, v));
        double s[3] = {s0, u * s0, v * s0};
        if (!(s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0)) continue;          // false for a NaN
        if (!(__builtin_isfinite(s[0]) && __builtin_isfinite(s[1]) && __builtin_isfinite(s[2]))) continue;
        // Gauss-Newton on g(s) = the three law-of-cosines residuals
#pragma unroll 1
        for (int it = 0; it < P3P_POLISH; ++it) {
            const double g0 = (s[1] * s[1] + s[2] * s[2]) - 2.0 * s[1] * s[2] * ca - a2;
            const double g1 = (s[0] * s[0] + s[2] * s[2]) - 2.0 * s[0] * s[2] * cb - b2;
            const double g2 = (s[0] * s[0] + s[1] * s[1]) - 2.0 * s[0] * s[1] * cg - c2;
            const double J[3][3] = {{0.0, 2.0 * (s[1] - s[2] * ca), 2.0 * (s[2] - s[1] * ca)},
                                    {2.0 * (s[0] - s[2] * cb), 0.0, 2.0 * (s[2] - s[0] * cb)},
                                    {2.0 * (s[0] - s[1] * cg), 2.0 * (s[1] - s[0] * cg), 0.0}};
            double gv[3] = {g0, g1, g2};
            const double det = p3p_det3(J, nullptr, -1);
            const double d0 = p3p_det3(J, gv, 0), d1 = p3p_det3(J, gv, 1), d2 = p3p_det3(J, gv, 2);         // Cramer: J d = g
            const double t0 = s[0] - d0 / det, t1 = s[1] - d1 / det, t2 = s[2] - d2 / det;
            const double h0 = (t1 * t1 + t2 * t2) - 2.0 * t1 * t2 * ca - a2, h1 = (t0 * t0 + t2 * t2) - 2.0 * t0 * t2 * cb - b2,
                         h2 = (t0 * t0 + t1 * t1) - 2.0 * t0 * t1 * cg - c2;
            const bool better = (h0 * h0 + h1 * h1) + h2 * h2 < (g0 * g0 + g1 * g1) + g2 * g2 && t0 > 0.0 && t1 > 0.0 && t2 > 0.0;
            if (!better) break;                         // also for a NaN step
            s[0] = t0; s[1] = t1; s[2] = t2;
        }
        double Y[3][3], FX[3][3], FY[3][3];
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) Y[i][k] = s[i] * f[i][k];
        p3p_frame(X, FX);
        p3p_frame(Y, FY);
        double R[9], t[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i * 3 + j] = (FY[0][i] * FX[0][j] + FY[1][i] * FX[1][j]) + FY[2][i] * FX[2][j];
        for (int i = 0; i < 3; ++i) t[i] = Y[0][i] - ((R[i * 3] * X[0][0] + R[i * 3 + 1] * X[0][1]) + R[i * 3 + 2] * X[0][2]);
        bool ok = true;
        for (int k = 0; k < 9; ++k) ok = ok && __builtin_isfinite(R[k]) && __builtin_isfinite((double)(float)R[k]);
        for (int k = 0; k < 3; ++k) ok = ok && __builtin_isfinite(t[k]) && __builtin_isfinite((double)(float)t[k]);
        double worst = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double y0 = ((R[0] * X[i][0] + R[1] * X[i][1]) + R[2] * X[i][2]) + t[0], y1 = ((R[3] * X[i][0] + R[4] * X[i][1]) + R[5] * X[i][2]) + t[1],
                         y2 = ((R[6] * X[i][0] + R[7] * X[i][1]) + R[8] * X[i][2]) + t[2];
            ok = ok && y2 > 0.0;
            const double e0 = __builtin_fabs(y0 / y2 - r[i][0]), e1 = __builtin_fabs(y1 / y2 - r[i][1]);
            worst = e0 > worst ? e0 : worst;
            worst = e1 > worst ? e1 : worst;
            ok = ok && __builtin_isfinite(e0) && __builtin_isfinite(e1);
        }
        ok = ok && worst <= P3P_SELF_CHECK;
        if (!ok || n >= 4) continue;
        // insertion by ascending s_0 (a later equal distance stays behind)
        int at = n;
        while (at > 0 && s0s[at - 1] > s[0]) {
            s0s[at] = s0s[at - 1];
            for (int k = 0; k < 12; ++k) Rt[at][k] = Rt[at - 1][k];
            --at;
        }
        s0s[at] = s[0];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) Rt[at][i * 4 + j] = R[i * 3 + j];
            Rt[at][i * 4 + 3] = t[i];
        }
        ++n;
    }
    return n;
}

}  // namespace pats
