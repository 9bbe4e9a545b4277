/* mlpnp_core.h -- the scalar algebra of MLPnPsolver (src/MLPnPsolver.cpp:395-851) in one text for both sides: mlpnp.hip includes it for the
 * device, tests/mlpnp_ref/mlpnp_ref.c for the CPU restatement.  It is the C / C++ common subset, strict IEEE (-ffp-contract=off on both
 * sides), and whatever is indexed at run time sits in memory the caller hands in (LDS on the device); the few local arrays are indexed by
 * unrolled constants and stay in registers, so the device needs no scratch.  What the
 * two sides write separately is everything that has a shape: the loops over correspondences, sets and iterations, the lanes, the sums
 * over rows, the result rule.  Eigen 3.3's algorithms are restated on their scalar paths; DESIGN.md section 2, "Parity choices of the
 * MLPnP solver", lists each reading.  None is pinned against a build of the reference.
 *
 * The includer defines, before the include:
 *   MLP_FN                     the function qualifier
 *   MLP_SINCOS(x, ps, pc)      double sin / cos (dev_dsincos's text; a NaN handed through)
 *   MLP_HI(x) MLP_LO(x)        the high / low word of a double as int32_t / uint32_t;  MLP_MK(hi, lo) the double of two words
 *   MLP_PROBE(id)              optional: counts a branch (the restatement's branch probe); nothing on the device
 *   MLP_ACOS(x) MLP_CBRT(x)    optional: acos and pow(x, 1.0/3.0); default dev_dacos / dev_dpow below
 */
#ifndef MLPNP_CORE_H
#define MLPNP_CORE_H

#ifndef MLP_PROBE
#define MLP_PROBE(id) ((void)0)
#endif
#ifndef MLP_ACOS
#define MLP_ACOS(x) dev_dacos(x)
#endif
#ifndef MLP_CBRT
#define MLP_CBRT(x) dev_dpow((x), 1.0 / 3.0)
#endif

enum {
    MLPP_PLANAR, MLPP_NONPLANAR, MLPP_DET_FLIP_1, MLPP_DET_KEEP_1, MLPP_DET_FLIP_2, MLPP_DET_KEEP_2, MLPP_PLANAR_CHOICE /* 4 */,
    MLPP_NONPLANAR_CHOICE = MLPP_PLANAR_CHOICE + 4 /* 2 */, MLPP_GN_EXIT_DL = MLPP_NONPLANAR_CHOICE + 2, MLPP_GN_EXIT_MAXIT, MLPP_GN_EXIT_DX,
    MLPP_LDLT_MOVED, MLPP_LDLT_KEPT, MLPP_RODRIGUES_ZERO, MLPP_RODRIGUES_GENERAL, MLPP_ROT_IDENTITY, MLPP_ROT_GENERAL, MLPP_HOUSEHOLDER_ZERO,
    MLPP_HOUSEHOLDER_GENERAL, MLPP_SVD_NO_ROTATION, MLPP_SVD_ROTATION, MLPP_SVD_SWAP, MLPP_EIG_V1_ZERO, MLPP_EIG_V1_GENERAL, MLPP_TOO_FEW,
    MLPP_REFINED, MLPP_BEST_RETURNED, MLPP_NOTHING_RETURNED, MLPP_PINHOLE, MLPP_KB8, MLPP_N
};

#define MLP_DBL_MIN 2.2250738585072014e-308
#define MLP_DBL_EPS 2.2204460492503131e-16

/* ---- fdlibm e_acos.c and e_pow.c (x >= 0 or NaN, 0 < y <= 0.5: no overflow, no subnormal result) ------------------------------------ */
MLP_FN double dev_dacos(double x)
{
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const int32_t hx = MLP_HI(x), ix = hx & 0x7fffffff;
    double z, p, q, r, w, s, c, df;
    if (ix >= 0x3ff00000) {
        if ((((uint32_t)ix - 0x3ff00000u) | MLP_LO(x)) == 0) return hx > 0 ? 0.0 : pi + 2.0 * pio2_lo;
        return (x - x) / (x - x);
    }
    if (ix < 0x3fe00000) {
        if (ix <= 0x3c600000) return pio2_hi + pio2_lo;
        z = x * x;
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        r = p / q;
        return pio2_hi - (x - (pio2_lo - r * x));
    }
    if (hx < 0) {
        z = (1.0 + x) * 0.5;
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        s = sqrt(z);
        r = p / q;
        w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    z = (1.0 - x) * 0.5;
    s = sqrt(z);
    df = MLP_MK(MLP_HI(s), 0u);
    c = (z - df * df) / (s + df);
    p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    r = p / q;
    w = r * s + c;
    return 2.0 * (df + w);
}
MLP_FN double dev_dpow(double x, double y)
{
    const double two53 = 9007199254740992.0;
    const double L1 = 5.99999999999994648725e-01, L2 = 4.28571428578550184252e-01, L3 = 3.33333329818377432918e-01,
                 L4 = 2.72728123808534006489e-01, L5 = 2.30660745775561754067e-01, L6 = 2.06975017800338417784e-01,
                 P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
                 P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08, lg2 = 6.93147180559945286227e-01,
                 lg2_h = 6.93147182464599609375e-01, lg2_l = -1.90465429995776804525e-09, cp = 9.61796693925975554329e-01,
                 cp_h = 9.61796700954437255859e-01, cp_l = -7.02846165095275826516e-09;
    if (x != x || y != y) return x + y;
    if (x == 0.0) return 0.0;
    if (MLP_HI(x) >= 0x7ff00000) return x;                          /* +inf */
    double ax = x, u, v, ss, s_h, s_l, t_h, t_l, s2, r, p_h, p_l, z_h, z_l, t, t1, t2, y1, z, w;
    int32_t hx = MLP_HI(ax), n = 0, j, ix, k, i;
    if (hx < 0x00100000) { ax *= two53; n -= 53; hx = MLP_HI(ax); }
    n += (hx >> 20) - 0x3ff;
    j = hx & 0x000fffff;
    ix = j | 0x3ff00000;
    if (j <= 0x3988E) k = 0;
    else if (j < 0xBB67A) k = 1;
    else { k = 0; n += 1; ix -= 0x00100000; }
    ax = MLP_MK(ix, MLP_LO(ax));
    const double bpk = k ? 1.5 : 1.0, dp_h = k ? 5.84962487220764160156e-01 : 0.0, dp_l = k ? 1.35003920212974897128e-08 : 0.0;
    u = ax - bpk;
    v = 1.0 / (ax + bpk);
    ss = u * v;
    s_h = MLP_MK(MLP_HI(ss), 0u);
    t_h = MLP_MK(((ix >> 1) | 0x20000000) + 0x00080000 + (k << 18), 0u);
    t_l = ax - (t_h - bpk);
    s_l = v * ((u - s_h * t_h) - s_h * t_l);
    s2 = ss * ss;
    r = s2 * s2 * (L1 + s2 * (L2 + s2 * (L3 + s2 * (L4 + s2 * (L5 + s2 * L6)))));
    r += s_l * (s_h + ss);
    s2 = s_h * s_h;
    t_h = 3.0 + s2 + r;
    t_h = MLP_MK(MLP_HI(t_h), 0u);
    t_l = r - ((t_h - 3.0) - s2);
    u = s_h * t_h;
    v = s_l * t_h + t_l * ss;
    p_h = u + v;
    p_h = MLP_MK(MLP_HI(p_h), 0u);
    p_l = v - (p_h - u);
    z_h = cp_h * p_h;
    z_l = cp_l * p_h + p_l * cp + dp_l;
    t = (double)n;
    t1 = (((z_h + z_l) + dp_h) + t);
    t1 = MLP_MK(MLP_HI(t1), 0u);
    t2 = z_l - (((t1 - t) - dp_h) - z_h);
    y1 = MLP_MK(MLP_HI(y), 0u);
    p_l = (y - y1) * t1 + y * t2;
    p_h = y1 * t1;
    z = p_l + p_h;
    j = MLP_HI(z);
    i = j & 0x7fffffff;
    k = (i >> 20) - 0x3ff;
    n = 0;
    if (i > 0x3fe00000) {
        n = j + (0x00100000 >> (k + 1));
        k = ((n & 0x7fffffff) >> 20) - 0x3ff;
        t = MLP_MK(n & ~(0x000fffff >> k), 0u);
        n = ((n & 0x000fffff) | 0x00100000) >> (20 - k);
        if (j < 0) n = -n;
        p_h -= t;
    }
    t = p_l + p_h;
    t = MLP_MK(MLP_HI(t), 0u);
    u = t * lg2_h;
    v = (p_l - (t - p_h)) * lg2 + t * lg2_l;
    z = u + v;
    w = v - (z - u);
    t = z * z;
    t1 = z - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    r = (z * t1) / (t1 - 2.0) - (w + z * w);
    z = 1.0 - (r - z);
    return MLP_MK(MLP_HI(z) + (int32_t)((uint32_t)n << 20), MLP_LO(z));
}

/* ---- Householder::makeHouseholder of v[0..n) in place: v[0] <- beta, v[1..) <- the essential part; returns tau ----------------------- */
MLP_FN double mlp_make_householder(double* v, int n, int stride)
{
    double tail = 0.0;
    for (int i = 1; i < n; i++) tail += v[i * stride] * v[i * stride];
    const double c0 = v[0];
    if (tail <= MLP_DBL_MIN) {
        MLP_PROBE(MLPP_HOUSEHOLDER_ZERO);
        for (int i = 1; i < n; i++) v[i * stride] = 0.0;
        return 0.0;
    }
    MLP_PROBE(MLPP_HOUSEHOLDER_GENERAL);
    double beta = sqrt(c0 * c0 + tail);
    if (c0 >= 0.0) beta = -beta;
    for (int i = 1; i < n; i++) v[i * stride] = v[i * stride] / (c0 - beta);
    v[0] = beta;
    return (beta - c0) / beta;
}

/* the nullspace of one bearing vector (:410-412): JacobiSVD<MatrixXd, HouseholderQRPreconditioner>(f^T, ComputeFullV): the 1x3 is scaled
 * by its largest |entry| (first entry first, replaced on >), its adjoint gets one reflector, V is the full Q (the reflector applied to
 * the identity from the left), and the 1x1 work matrix needs no sweep.  ns[6] = columns 1 and 2 of V, row-major 3x2. */
MLP_FN void mlp_nullspace(const double* f, double* ns)
{
    double scale = fabs(f[0]);
    if (fabs(f[1]) > scale) scale = fabs(f[1]);
    if (fabs(f[2]) > scale) scale = fabs(f[2]);
    if (scale == 0.0) scale = 1.0;
    const double c0 = f[0] / scale, e1 = f[1] / scale, e2 = f[2] / scale;
    const double tail = e1 * e1 + e2 * e2;
    if (tail <= MLP_DBL_MIN) {
        MLP_PROBE(MLPP_HOUSEHOLDER_ZERO);
        ns[0] = 0.0; ns[1] = 0.0; ns[2] = 1.0; ns[3] = 0.0; ns[4] = 0.0; ns[5] = 1.0;
        return;
    }
    MLP_PROBE(MLPP_HOUSEHOLDER_GENERAL);
    double beta = sqrt(c0 * c0 + tail);
    if (c0 >= 0.0) beta = -beta;
    const double es1 = e1 / (c0 - beta), es2 = e2 / (c0 - beta), tau = (beta - c0) / beta;
    /* applyHouseholderOnTheLeft on the identity, columns j = 1, 2: tmp = essential^T * bottom + row 0 */
    const double t1 = (es1 * 1.0 + es2 * 0.0) + 0.0, t2 = (es1 * 0.0 + es2 * 1.0) + 0.0;
    ns[0] = 0.0 - tau * t1;              ns[1] = 0.0 - tau * t2;
    ns[2] = 1.0 - (tau * es1) * t1;      ns[3] = 0.0 - (tau * es1) * t2;
    ns[4] = 0.0 - (tau * es2) * t1;      ns[5] = 1.0 - (tau * es2) * t2;
}

/* FullPivHouseholderQR<Matrix3d>(M).rank(), default threshold 3*eps; M (row-major 3x3) is destroyed */
MLP_FN int mlp_rank3(double* m)
{
    const double precision = MLP_DBL_EPS * 3.0;
    int nonzero = 3;
    double maxpivot = 0.0, biggest = 0.0;
    for (int k = 0; k < 3; k++) {
        int br = k, bc = k;
        double score = fabs(m[3 * k + k]);
        for (int j = k; j < 3; j++)                   /* column-major visit, replaced on > */
            for (int i = k; i < 3; i++)
                if (fabs(m[3 * i + j]) > score) { score = fabs(m[3 * i + j]); br = i; bc = j; }
        if (k == 0) biggest = score;
        if (fabs(score) <= fabs(biggest) * precision) { nonzero = k; break; }
        if (br != k) for (int j = k; j < 3; j++) { const double t = m[3 * k + j]; m[3 * k + j] = m[3 * br + j]; m[3 * br + j] = t; }
        if (bc != k) for (int i = 0; i < 3; i++) { const double t = m[3 * i + k]; m[3 * i + k] = m[3 * i + bc]; m[3 * i + bc] = t; }
        const double tau = mlp_make_householder(m + 3 * k + k, 3 - k, 3);
        const double beta = m[3 * k + k];
        if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
        if (3 - k > 1 && tau != 0.0)
            for (int j = k + 1; j < 3; j++) {
                double tmp = 0.0;
                for (int i = k + 1; i < 3; i++) tmp += m[3 * i + k] * m[3 * i + j];
                tmp += m[3 * k + j];
                m[3 * k + j] -= tau * tmp;
                for (int i = k + 1; i < 3; i++) m[3 * i + j] -= (tau * m[3 * i + k]) * tmp;
            }
    }
    const double thr = fabs(maxpivot) * precision;
    int rank = 0;
    for (int i = 0; i < nonzero; i++) rank += fabs(m[3 * i + i]) > thr;
    return rank;
}

/* JacobiRotation::makeGivens, real */
MLP_FN void mlp_givens(double p, double q, double* c, double* s)
{
    if (q == 0.0) { *c = p < 0.0 ? -1.0 : 1.0; *s = 0.0; }
    else if (p == 0.0) { *c = 0.0; *s = q < 0.0 ? 1.0 : -1.0; }
    else if (fabs(p) > fabs(q)) {
        const double t = q / p;
        double u = sqrt(1.0 + t * t);
        if (p < 0.0) u = -u;
        *c = 1.0 / u; *s = -t * *c;
    } else {
        const double t = p / q;
        double u = sqrt(1.0 + t * t);
        if (q < 0.0) u = -u;
        *s = -1.0 / u; *c = -t * *s;
    }
}

/* SelfAdjointEigenSolver<Matrix3d>::compute (the iterative one) of the lower triangle of M: eigenvalues increasing in w[3], the
 * eigenvectors as the columns of Q (row-major 3x3).  The sort is skipped when the 90 iterations run out, as in the source. */
MLP_FN void mlp_eig3(const double* M, double* w, double* Q, double* sub)
{
    double a00 = M[0], a10 = M[3], a11 = M[4], a20 = M[6], a21 = M[7], a22 = M[8];
    double scale = fabs(a00);                         /* column-major visit of the lower triangle (the upper one is zero) */
    if (fabs(a10) > scale) scale = fabs(a10);
    if (fabs(a20) > scale) scale = fabs(a20);
    if (fabs(a11) > scale) scale = fabs(a11);
    if (fabs(a21) > scale) scale = fabs(a21);
    if (fabs(a22) > scale) scale = fabs(a22);
    if (scale == 0.0) scale = 1.0;
    a00 /= scale; a10 /= scale; a11 /= scale; a20 /= scale; a21 /= scale; a22 /= scale;
    /* tridiagonalization_inplace, the 3x3 real form */
    w[0] = a00;
    const double v1norm2 = a20 * a20;
    if (v1norm2 <= MLP_DBL_MIN) {
        MLP_PROBE(MLPP_EIG_V1_ZERO);
        w[1] = a11; w[2] = a22; sub[0] = a10; sub[1] = a21;
        for (int i = 0; i < 9; i++) Q[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
        MLP_PROBE(MLPP_EIG_V1_GENERAL);
        const double beta = sqrt(a10 * a10 + v1norm2), invBeta = 1.0 / beta, m01 = a10 * invBeta, m02 = a20 * invBeta;
        const double q = 2.0 * m01 * a21 + m02 * (a22 - a11);
        w[1] = a11 + m02 * q; w[2] = a22 - m02 * q; sub[0] = beta; sub[1] = a21 - m01 * q;
        Q[0] = 1.0; Q[1] = 0.0; Q[2] = 0.0; Q[3] = 0.0; Q[4] = m01; Q[5] = m02; Q[6] = 0.0; Q[7] = m02; Q[8] = -m01;
    }
    /* computeFromTridiagonal_impl */
    int end = 2, start = 0, iter = 0;
    const double precision = 2.0 * MLP_DBL_EPS;
    while (end > 0) {
        for (int i = start; i < end; i++)
            if (fabs(sub[i]) <= (fabs(w[i]) + fabs(w[i + 1])) * precision || fabs(sub[i]) <= MLP_DBL_MIN) sub[i] = 0.0;
        while (end > 0 && sub[end - 1] == 0.0) end--;
        if (end <= 0) break;
        iter++;
        if (iter > 30 * 3) break;
        start = end - 1;
        while (start > 0 && sub[start - 1] != 0.0) start--;
        /* tridiagonal_qr_step */
        const double td = (w[end - 1] - w[end]) * 0.5, e = sub[end - 1];
        double mu = w[end];
        if (td == 0.0) mu -= fabs(e);
        else {
            const double e2 = e * e;
            const double ax = fabs(td), ay = fabs(e), p = ax > ay ? ax : ay, qp = (ay < ax ? ay : ax) / p, h = p * sqrt(1.0 + qp * qp);
            if (e2 == 0.0) mu -= (e / (td + (td > 0.0 ? 1.0 : -1.0))) * (e / h);
            else mu -= e2 / (td + (td > 0.0 ? h : -h));
        }
        double x = w[start] - mu, z = sub[start];
        for (int k = start; k < end; k++) {
            double c, s;
            mlp_givens(x, z, &c, &s);
            const double sdk = s * w[k] + c * sub[k], dkp1 = s * sub[k] + c * w[k + 1];
            w[k] = c * (c * w[k] - s * sub[k]) - s * (c * sub[k] - s * w[k + 1]);
            w[k + 1] = s * sdk + c * dkp1;
            sub[k] = c * sdk - s * dkp1;
            if (k > start) sub[k - 1] = c * sub[k - 1] - s * z;
            x = sub[k];
            if (k < end - 1) { z = -s * sub[k + 1]; sub[k + 1] = c * sub[k + 1]; }
            if (!(c == 1.0 && s == 0.0))
                for (int i = 0; i < 3; i++) {         /* Q.applyOnTheRight(k, k+1, rot): the plane rotation (c, -s) on two columns */
                    const double xi = Q[3 * i + k], yi = Q[3 * i + k + 1];
                    Q[3 * i + k] = c * xi - s * yi;
                    Q[3 * i + k + 1] = s * xi + c * yi;
                }
        }
    }
    if (iter <= 30 * 3)
        for (int i = 0; i < 2; i++) {
            int k = 0;
            for (int j = 1; j < 3 - i; j++) if (w[i + j] < w[i + k]) k = j;
            if (k > 0) {
                const double t = w[i]; w[i] = w[i + k]; w[i + k] = t;
                for (int r = 0; r < 3; r++) { const double u = Q[3 * r + i]; Q[3 * r + i] = Q[3 * r + i + k]; Q[3 * r + i + k] = u; }
            }
        }
    w[0] *= scale; w[1] *= scale; w[2] *= scale;
}

/* ---- JacobiSVD of a square matrix (no preconditioner): the pieces both sides share.  W is the work matrix (already divided by the
 * scale), row-major with stride n. ------------------------------------------------------------------------------------------------- */
typedef struct { double lc, ls, rc, rs; } mlp_rot2;
/* real_2x2_jacobi_svd of (W[p][p], W[p][q]; W[q][p], W[q][q]) -> j_left (lc, ls), j_right (rc, rs) */
MLP_FN mlp_rot2 mlp_svd2x2(double m00, double m01, double m10, double m11)
{
    mlp_rot2 o;
    double c1, s1;
    const double t = m00 + m11, d = m10 - m01;
    if (fabs(d) < MLP_DBL_MIN) { s1 = 0.0; c1 = 1.0; }
    else { const double u = t / d, tmp = sqrt(1.0 + u * u); s1 = 1.0 / tmp; c1 = u / tmp; }
    if (!(c1 == 1.0 && s1 == 0.0)) {                  /* m.applyOnTheLeft(0, 1, rot1) */
        const double x0 = m00, y0 = m10, x1 = m01, y1 = m11;
        m00 = c1 * x0 + s1 * y0; m10 = -s1 * x0 + c1 * y0;
        m01 = c1 * x1 + s1 * y1; m11 = -s1 * x1 + c1 * y1;
    }
    /* j_right->makeJacobi(m(0,0), m(0,1), m(1,1)) */
    const double deno = 2.0 * fabs(m01);
    if (deno < MLP_DBL_MIN) { o.rc = 1.0; o.rs = 0.0; }
    else {
        const double tau = (m00 - m11) / deno, w = sqrt(tau * tau + 1.0);
        const double tt = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
        const double sign_t = tt > 0.0 ? 1.0 : -1.0, n = 1.0 / sqrt(tt * tt + 1.0);
        o.rs = -sign_t * (m01 / fabs(m01)) * fabs(tt) * n;
        o.rc = n;
    }
    /* *j_left = rot1 * j_right->transpose() */
    o.lc = c1 * o.rc - s1 * (-o.rs);
    o.ls = c1 * (-o.rs) + s1 * o.rc;
    return o;
}
/* the four plane rotations of one (p, q) step on element i of a row / column.  Left on W: rows p, q at column i.  Right on W and V:
 * columns p, q at row i.  U: columns p, q at row i with j_left. */
#define MLP_ROT_LEFT(M, n, p, q, i, c, s) do { if (!((c) == 1.0 && (s) == 0.0)) { const double xi_ = M[(p) * (n) + (i)], yi_ = M[(q) * (n) + (i)]; \
        M[(p) * (n) + (i)] = (c) * xi_ + (s) * yi_; M[(q) * (n) + (i)] = -(s) * xi_ + (c) * yi_; } } while (0)
#define MLP_ROT_RIGHT(M, n, p, q, i, c, s) do { if (!((c) == 1.0 && (s) == 0.0)) { const double xi_ = M[(i) * (n) + (p)], yi_ = M[(i) * (n) + (q)]; \
        M[(i) * (n) + (p)] = (c) * xi_ - (s) * yi_; M[(i) * (n) + (q)] = (s) * xi_ + (c) * yi_; } } while (0)
#define MLP_ROT_U(M, n, p, q, i, c, s) do { if (!((c) == 1.0 && (s) == 0.0)) { const double xi_ = M[(i) * (n) + (p)], yi_ = M[(i) * (n) + (q)]; \
        M[(i) * (n) + (p)] = (c) * xi_ + (s) * yi_; M[(i) * (n) + (q)] = -(s) * xi_ + (c) * yi_; } } while (0)

/* the scale: the largest |entry|, column-major visit, first entry first, replaced on > (a NaN first entry stays) */
MLP_FN double mlp_svd_scale(const double* A, int n)
{
    double scale = fabs(A[0]);
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++)
            if (fabs(A[i * n + j]) > scale) scale = fabs(A[i * n + j]);
    if (scale == 0.0) scale = 1.0;
    return scale;
}
MLP_FN double mlp_svd_maxdiag(const double* W, int n)
{
    double m = fabs(W[0]);
    for (int i = 1; i < n; i++) if (fabs(W[i * n + i]) > m) m = fabs(W[i * n + i]);
    return m;
}
/* steps 3 and 4 after the sweeps: sv[i] = |W[i][i]|, the sign into U's column, times the scale, the descending sort by column swaps
 * (the first maximum wins; the sort ends at the first zero maximum) */
MLP_FN void mlp_svd_finish(const double* W, double* V, double* U, double* sv, int n, double scale)
{
    for (int i = 0; i < n; i++) {
        const double a = fabs(W[i * n + i]);
        sv[i] = a;
        if (U && a != 0.0) { const double f = W[i * n + i] / a; for (int r = 0; r < n; r++) U[r * n + i] *= f; }
    }
    for (int i = 0; i < n; i++) sv[i] *= scale;
    for (int i = 0; i < n; i++) {
        int pos = 0;
        double mx = sv[i];
        for (int j = 1; j < n - i; j++) if (sv[i + j] > mx) { mx = sv[i + j]; pos = j; }
        if (mx == 0.0) break;
        if (pos) {
            MLP_PROBE(MLPP_SVD_SWAP);
            pos += i;
            const double t = sv[i]; sv[i] = sv[pos]; sv[pos] = t;
            for (int r = 0; r < n; r++) {
                if (U) { const double u = U[r * n + pos]; U[r * n + pos] = U[r * n + i]; U[r * n + i] = u; }
                const double v = V[r * n + pos]; V[r * n + pos] = V[r * n + i]; V[r * n + i] = v;
            }
        }
    }
}
/* the whole SVD on one thread: A (n x n) -> W (destroyed work matrix), V, U (or NULL), sv; returns the rotations executed */
MLP_FN int mlp_jsvd(const double* A, int n, double* W, double* V, double* U, double* sv)
{
    const double precision = 2.0 * MLP_DBL_EPS, considerAsZero = 2.0 * 4.9406564584124654e-324;
    const double scale = mlp_svd_scale(A, n);
    int rotations = 0;
    for (int i = 0; i < n * n; i++) { W[i] = A[i] / scale; V[i] = (i % (n + 1) == 0) ? 1.0 : 0.0; if (U) U[i] = V[i]; }
    double maxDiag = mlp_svd_maxdiag(W, n);
    int finished = 0;
    while (!finished) {
        finished = 1;
        for (int p = 1; p < n; p++)
            for (int q = 0; q < p; q++) {
                const double thr0 = precision * maxDiag, threshold = considerAsZero > thr0 ? considerAsZero : thr0;
                if (fabs(W[p * n + q]) > threshold || fabs(W[q * n + p]) > threshold) {
                    finished = 0;
                    rotations++;
                    const mlp_rot2 r = mlp_svd2x2(W[p * n + p], W[p * n + q], W[q * n + p], W[q * n + q]);
                    for (int i = 0; i < n; i++) MLP_ROT_LEFT(W, n, p, q, i, r.lc, r.ls);
                    if (U) for (int i = 0; i < n; i++) MLP_ROT_U(U, n, p, q, i, r.lc, r.ls);
                    for (int i = 0; i < n; i++) MLP_ROT_RIGHT(W, n, p, q, i, r.rc, r.rs);
                    for (int i = 0; i < n; i++) MLP_ROT_RIGHT(V, n, p, q, i, r.rc, r.rs);
                    const double a = fabs(W[p * n + p]), b = fabs(W[q * n + q]), ab = a > b ? a : b;
                    if (ab > maxDiag) maxDiag = ab;
                }
            }
    }
    if (rotations) MLP_PROBE(MLPP_SVD_ROTATION); else MLP_PROBE(MLPP_SVD_NO_ROTATION);
    mlp_svd_finish(W, V, U, sv, n, scale);
    return rotations;
}

/* ---- 3x3 helpers, row-major; products with k ascending ---------------------------------------------------------------------------- */
MLP_FN double mlp_det3(const double* m)
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
MLP_FN void mlp_mul33(const double* a, const double* b, double* d)      /* d = a*b */
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) d[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
MLP_FN void mlp_mul33_bt(const double* a, const double* b, double* d)   /* d = a*b^T */
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) d[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}
MLP_FN void mlp_mul33_at(const double* a, const double* b, double* d)   /* d = a^T*b */
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) d[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}
MLP_FN void mlp_transpose3(double* m)
{
    double t;
    t = m[1]; m[1] = m[3]; m[3] = t;  t = m[2]; m[2] = m[6]; m[6] = t;  t = m[5]; m[5] = m[7]; m[7] = t;
}
MLP_FN double mlp_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }
/* sum over the first six correspondences of 1 - (R*X + t)/|R*X + t| . f (:622-631, :668-672) */
MLP_FN double mlp_direction_error(const double* R, const double* t, const double* X6, const double* f6)
{
    double err = 0.0;
    for (int p = 0; p < 6; p++) {
        const double* X = X6 + 3 * p;
        double v0 = (R[0] * X[0] + R[1] * X[1] + R[2] * X[2]) + t[0], v1 = (R[3] * X[0] + R[4] * X[1] + R[5] * X[2]) + t[1],
               v2 = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2]) + t[2];
        const double nv = mlp_norm3(v0, v1, v2);
        v0 = v0 / nv; v1 = v1 / nv; v2 = v2 / nv;
        err += (1.0 - (v0 * f6[3 * p] + v1 * f6[3 * p + 1] + v2 * f6[3 * p + 2]));
    }
    return err;
}

/* rodrigues2rot (:703-718) */
MLP_FN void mlp_rodrigues2rot(const double* om, double* R)
{
    const double n = mlp_norm3(om[0], om[1], om[2]);
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (n > MLP_DBL_EPS) {
        MLP_PROBE(MLPP_ROT_GENERAL);
        /* |omega| <= pi + 5*5*sqrt(3) < 100: acos gives at most pi, five steps add at most 5 per entry each (the dx guard) */
        double sn, cs;
        MLP_SINCOS(n, &sn, &cs);
        const double a = sn / n, b = (1.0 - cs) / (n * n);
        const double K[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double kk = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
                R[3 * i + j] = (R[3 * i + j] + a * K[3 * i + j]) + b * kk;
            }
    } else MLP_PROBE(MLPP_ROT_IDENTITY);
}
/* rot2rodrigues (:720-735) */
MLP_FN void mlp_rot2rodrigues(const double* R, double* om)
{
    om[0] = 0.0; om[1] = 0.0; om[2] = 0.0;
    const double trace = ((R[0] + R[4]) + R[8]) - 1.0;
    const double wnorm = MLP_ACOS(trace / 2.0);
    if (wnorm > MLP_DBL_EPS) {
        MLP_PROBE(MLPP_RODRIGUES_GENERAL);
        double sn, cs;
        MLP_SINCOS(wnorm, &sn, &cs);
        const double sc = wnorm / (2.0 * sn);
        om[0] = (R[7] - R[5]) * sc; om[1] = (R[2] - R[6]) * sc; om[2] = (R[3] - R[1]) * sc;
    } else MLP_PROBE(MLPP_RODRIGUES_ZERO);
}

/* one entry of a row of the design matrix A (:480-552): row 2i + j of correspondence i, column c.  pt is the point (rotated into the
 * eigen frame when planar) as three scalars, ns its nullspace (row-major 3x2). */
MLP_FN double mlp_design(int planar, const double* ns, double p0, double p1, double p2, int j, int c)
{
    if (planar) return c < 6 ? ns[2 * (c >> 1) + j] * ((c & 1) ? p2 : p1) : ns[2 * (c - 6) + j];
    if (c >= 9) return ns[2 * (c - 9) + j];
    const int m = c % 3;
    return ns[2 * (c / 3) + j] * (m == 0 ? p0 : m == 1 ? p1 : p2);
}

/* from the last right singular vector to the start of the Gauss-Newton refinement (:574-692): x[6] = (omega, t).  X6 / f6: the first
 * six correspondences (points3v, not rotated).  ws: 64 doubles of work space. */
MLP_FN void mlp_recover_pose(int planar, const double* res1, const double* eigenRot, const double* X6, const double* f6, double* x, double* ws)
{
    double* tmp = ws;          /* 9 */
    double* W = ws + 9;        /* 9 */
    double* V = ws + 18;       /* 9 */
    double* U = ws + 27;       /* 9 */
    double* Ro = ws + 36;      /* 9 */
    double* R2 = ws + 45;      /* 9 */
    double* sv = ws + 54;      /* 3 */
    double* t = ws + 57;       /* 3 */
    double* tn = ws + 60;      /* 3 */
    if (planar) {
        MLP_PROBE(MLPP_PLANAR);
        /* tmp << 0, r0, r1, 0, r2, r3, 0, r4, r5; column 0 = column 1 x column 2; transposed in place */
        const double a0 = res1[0], a1 = res1[2], a2 = res1[4], b0 = res1[1], b1 = res1[3], b2 = res1[5];
        const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
        tmp[0] = c0; tmp[1] = c1; tmp[2] = c2; tmp[3] = a0; tmp[4] = a1; tmp[5] = a2; tmp[6] = b0; tmp[7] = b1; tmp[8] = b2;
        const double scale = 1.0 / sqrt(fabs(mlp_norm3(tmp[1], tmp[4], tmp[7]) * mlp_norm3(tmp[2], tmp[5], tmp[8])));
        mlp_jsvd(tmp, 3, W, V, U, sv);
        mlp_mul33_bt(U, V, Ro);
        if (mlp_det3(Ro) < 0) { MLP_PROBE(MLPP_DET_FLIP_1); for (int i = 0; i < 9; i++) Ro[i] *= -1.0; } else MLP_PROBE(MLPP_DET_KEEP_1);
        mlp_mul33_at(eigenRot, Ro, R2);               /* Rout1 = eigenRot^T * Rout1 */
        t[0] = scale * res1[6]; t[1] = scale * res1[7]; t[2] = scale * res1[8];
        mlp_transpose3(R2);
        for (int i = 0; i < 9; i++) R2[i] *= -1.0;
        if (mlp_det3(R2) < 0.0) { MLP_PROBE(MLPP_DET_FLIP_2); R2[2] *= -1.0; R2[5] *= -1.0; R2[8] *= -1.0; } else MLP_PROBE(MLPP_DET_KEEP_2);
        /* the four combinations (R1, t), (R1, -t), (R2, t), (R2, -t), R2 = R1 with columns 0 and 1 negated; the first minimum wins */
        for (int i = 0; i < 9; i++) Ro[i] = (i % 3 == 2) ? R2[i] : -R2[i];
        tn[0] = -t[0]; tn[1] = -t[1]; tn[2] = -t[2];
        int idx = 0;
        double best = mlp_direction_error(R2, t, X6, f6);
        for (int i = 1; i < 4; i++) {
            const double e = mlp_direction_error(i < 2 ? R2 : Ro, (i & 1) ? tn : t, X6, f6);
            if (e < best) { best = e; idx = i; }
        }
        MLP_PROBE(MLPP_PLANAR_CHOICE + idx);
        const double* Rc = idx < 2 ? R2 : Ro;
        const double* tc = (idx & 1) ? tn : t;
        for (int i = 0; i < 9; i++) tmp[i] = Rc[i];
        x[3] = tc[0]; x[4] = tc[1]; x[5] = tc[2];
    } else {
        MLP_PROBE(MLPP_NONPLANAR);
        tmp[0] = res1[0]; tmp[1] = res1[3]; tmp[2] = res1[6]; tmp[3] = res1[1]; tmp[4] = res1[4]; tmp[5] = res1[7];
        tmp[6] = res1[2]; tmp[7] = res1[5]; tmp[8] = res1[8];
        const double prod = mlp_norm3(tmp[0], tmp[3], tmp[6]) * mlp_norm3(tmp[1], tmp[4], tmp[7]) * mlp_norm3(tmp[2], tmp[5], tmp[8]);
        const double scale = 1.0 / MLP_CBRT(fabs(prod));
        mlp_jsvd(tmp, 3, W, V, U, sv);
        mlp_mul33_bt(U, V, Ro);
        if (mlp_det3(Ro) < 0) { MLP_PROBE(MLPP_DET_FLIP_1); for (int i = 0; i < 9; i++) Ro[i] *= -1.0; } else MLP_PROBE(MLPP_DET_KEEP_1);
        const double s0 = scale * res1[9], s1 = scale * res1[10], s2 = scale * res1[11];
        t[0] = Ro[0] * s0 + Ro[1] * s1 + Ro[2] * s2; t[1] = Ro[3] * s0 + Ro[4] * s1 + Ro[5] * s2; t[2] = Ro[6] * s0 + Ro[7] * s1 + Ro[8] * s2;
        /* Ts[s] = (Rout, +-tout; 0 0 0 1).inverse(): Matrix4d::inverse() by cofactors.  With the last row (0, 0, 0, 1) the cofactors
         * of the upper-left block are those of Rout times 1 (their other two products hold a zero factor and are added as +-0), the
         * determinant is the sum col(0) . row(0) in the order (a + b) + (c + d) with d = 0 * cofactor. */
        double err[2];
        for (int s = 0; s < 2; s++) {
            const double tt[3] = {s ? -t[0] : t[0], s ? -t[1] : t[1], s ? -t[2] : t[2]};
            double m[16] = {Ro[0], Ro[1], Ro[2], tt[0], Ro[3], Ro[4], Ro[5], tt[1], Ro[6], Ro[7], Ro[8], tt[2], 0.0, 0.0, 0.0, 1.0};
            double inv[16];
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) {
                    const int i1 = (i + 1) & 3, i2 = (i + 2) & 3, i3 = (i + 3) & 3, j1 = (j + 1) & 3, j2 = (j + 2) & 3, j3 = (j + 3) & 3;
                    const double cof = (m[4 * i1 + j1] * (m[4 * i2 + j2] * m[4 * i3 + j3] - m[4 * i2 + j3] * m[4 * i3 + j2])
                                        + m[4 * i2 + j1] * (m[4 * i3 + j2] * m[4 * i1 + j3] - m[4 * i3 + j3] * m[4 * i1 + j2]))
                                       + m[4 * i3 + j1] * (m[4 * i1 + j2] * m[4 * i2 + j3] - m[4 * i1 + j3] * m[4 * i2 + j2]);
                    inv[4 * j + i] = ((i + j) & 1) ? -cof : cof;
                }
            const double det = (m[0] * inv[0] + m[4] * inv[1]) + (m[8] * inv[2] + m[12] * inv[3]);
            for (int i = 0; i < 16; i++) inv[i] /= det;
            double* Rs = s ? R2 : U;                  /* U is free after the product above */
            double* ts = s ? tn : sv;
            for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) Rs[3 * i + j] = inv[4 * i + j]; ts[i] = inv[4 * i + 3]; }
            err[s] = mlp_direction_error(Rs, ts, X6, f6);
        }
        const int pick = err[0] < err[1] ? 0 : 1;
        MLP_PROBE(MLPP_NONPLANAR_CHOICE + pick);
        const double* tc = pick ? tn : sv;
        x[3] = tc[0]; x[4] = tc[1]; x[5] = tc[2];
        for (int i = 0; i < 9; i++) tmp[i] = U[i];    /* Rout = Ts[0]'s rotation */
    }
    mlp_rot2rodrigues(tmp, x);
}

/* ---- the Gauss-Newton step (:737-851).  The Jacobian is the project's own derivation, not the reference's generated sequence:
 *   v = R(w) X + T, u = v/|v|, r_a = n_a . u;  dr_a/dv = g_a = (n_a - r_a u)/|v|;  dr_a/dT = g_a;
 *   d(R X)/dw_i = b_i x (R X),  b_i = (w_i w + w x ((I - R) e_i)) / (w . w)      (the derivative of the exponential map, Gallego & Yezzi 2015)
 * w = 0 gives 0/0 = NaN in every b_i, as the reference's 1/sqrt(0) does: the step is NaN and the hypothesis has no inliers. */
/* per step: R[9] and B[9] (b_i as rows) from x */
MLP_FN void mlp_gn_frame(const double* x, double* R, double* B)
{
    mlp_rodrigues2rot(x, R);
    const double th2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    for (int i = 0; i < 3; i++) {
        const double c0 = (i == 0 ? 1.0 : 0.0) - R[i], c1 = (i == 1 ? 1.0 : 0.0) - R[3 + i], c2 = (i == 2 ? 1.0 : 0.0) - R[6 + i];
        B[3 * i] = (x[i] * x[0] + (x[1] * c2 - x[2] * c1)) / th2;
        B[3 * i + 1] = (x[i] * x[1] + (x[2] * c0 - x[0] * c2)) / th2;
        B[3 * i + 2] = (x[i] * x[2] + (x[0] * c1 - x[1] * c0)) / th2;
    }
}
/* one correspondence: r[2] and J (two rows of 6, row a at J + 6a) */
MLP_FN void mlp_gn_point(const double* R, const double* B, const double* T, const double* X, const double* ns, double* r, double* J)
{
    const double q0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2], q1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2], q2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
    const double v0 = q0 + T[0], v1 = q1 + T[1], v2 = q2 + T[2];
    const double nv = mlp_norm3(v0, v1, v2), u0 = v0 / nv, u1 = v1 / nv, u2 = v2 / nv, inv = 1.0 / nv;
    for (int a = 0; a < 2; a++) {
        const double n0 = ns[a], n1 = ns[2 + a], n2 = ns[4 + a];
        const double ra = n0 * u0 + n1 * u1 + n2 * u2;
        const double g0 = (n0 - ra * u0) * inv, g1 = (n1 - ra * u1) * inv, g2 = (n2 - ra * u2) * inv;
        r[a] = ra;
        for (int i = 0; i < 3; i++) {
            const double b0 = B[3 * i], b1 = B[3 * i + 1], b2 = B[3 * i + 2];
            J[6 * a + i] = g0 * (b1 * q2 - b2 * q1) + g1 * (b2 * q0 - b0 * q2) + g2 * (b0 * q1 - b1 * q0);
        }
        J[6 * a + 3] = g0; J[6 * a + 4] = g1; J[6 * a + 5] = g2;
    }
}
/* LDLT<MatrixXd>(A).solve(g), 6x6: the pivoted unblocked factorisation of the lower triangle, in place in A (row-major); dx <- the
 * solution; tr: 6 ints of work space.  The dots and the substitutions run with the index ascending. */
MLP_FN void mlp_ldlt_solve(double* A, const double* g, double* dx, int* tr, double* temp)
{
    const int n = 6;
    int zero_diag = 0;
    for (int k = 0; k < n && !zero_diag; k++) {
        int big = 0;
        double mx = fabs(A[k * n + k]);
        for (int j = 1; j < n - k; j++) if (fabs(A[(k + j) * n + k + j]) > mx) { mx = fabs(A[(k + j) * n + k + j]); big = j; }
        big += k;
        tr[k] = big;
        if (k != big) {
            MLP_PROBE(MLPP_LDLT_MOVED);
            const int s = n - big - 1;
            for (int j = 0; j < k; j++) { const double t = A[k * n + j]; A[k * n + j] = A[big * n + j]; A[big * n + j] = t; }
            for (int i = n - s; i < n; i++) { const double t = A[i * n + k]; A[i * n + k] = A[i * n + big]; A[i * n + big] = t; }
            { const double t = A[k * n + k]; A[k * n + k] = A[big * n + big]; A[big * n + big] = t; }
            for (int i = k + 1; i < big; i++) { const double t = A[i * n + k]; A[i * n + k] = A[big * n + i]; A[big * n + i] = t; }
        } else MLP_PROBE(MLPP_LDLT_KEPT);
        const int rs = n - k - 1;
        if (k > 0) {
            for (int j = 0; j < k; j++) temp[j] = A[j * n + j] * A[k * n + j];
            double d = 0.0;
            for (int j = 0; j < k; j++) d += A[k * n + j] * temp[j];
            A[k * n + k] -= d;
            for (int i = k + 1; i < n; i++) {
                double s = 0.0;
                for (int j = 0; j < k; j++) s += A[i * n + j] * temp[j];
                A[i * n + k] -= s;
            }
        }
        const double akk = A[k * n + k];
        const int valid = fabs(akk) > 0.0;
        if (k == 0 && !valid) { for (int j = 0; j < n; j++) tr[j] = j; zero_diag = 1; break; }
        if (rs > 0 && valid) for (int i = k + 1; i < n; i++) A[i * n + k] /= akk;
    }
    for (int i = 0; i < n; i++) dx[i] = g[i];
    for (int k = 0; k < n; k++) if (tr[k] != k) { const double t = dx[k]; dx[k] = dx[tr[k]]; dx[tr[k]] = t; }
    for (int i = 0; i < n; i++)                       /* L y = P b, unit lower, column by column */
        for (int j = i + 1; j < n; j++) dx[j] -= dx[i] * A[j * n + i];
    for (int i = 0; i < n; i++) {
        if (fabs(A[i * n + i]) > 1.0 / 1.7976931348623157e+308) dx[i] /= A[i * n + i];
        else dx[i] = 0.0;
    }
    for (int i = n - 1; i >= 0; i--) {                /* L^T z = y, row by row */
        double s = 0.0;
        for (int j = i + 1; j < n; j++) s += A[j * n + i] * dx[j];
        dx[i] -= s;
    }
    for (int k = n - 1; k >= 0; k--) if (tr[k] != k) { const double t = dx[k]; dx[k] = dx[tr[k]]; dx[tr[k]] = t; }
}
/* dx.array().abs().maxCoeff() > 5.0 || dx.array().abs().minCoeff() > 1.0 (:788): the first entry first, replaced on > / < */
MLP_FN int mlp_gn_dx_guard(const double* dx)
{
    double mx = fabs(dx[0]), mn = fabs(dx[0]);
    for (int i = 1; i < 6; i++) { if (fabs(dx[i]) > mx) mx = fabs(dx[i]); if (fabs(dx[i]) < mn) mn = fabs(dx[i]); }
    return mx > 5.0 || mn > 1.0;
}

/* CheckInliers of one correspondence (:310-326): the camera point in double, narrowed to float; project; the strict < */
#define MLP_CAMERA_POINT(Rt, X, xc) do { \
        (xc)[0] = (float)((((Rt)[0] * (double)(X)[0] + (Rt)[1] * (double)(X)[1]) + (Rt)[2] * (double)(X)[2]) + (Rt)[9]); \
        (xc)[1] = (float)((((Rt)[3] * (double)(X)[0] + (Rt)[4] * (double)(X)[1]) + (Rt)[5] * (double)(X)[2]) + (Rt)[10]); \
        (xc)[2] = (float)((((Rt)[6] * (double)(X)[0] + (Rt)[7] * (double)(X)[1]) + (Rt)[8] * (double)(X)[2]) + (Rt)[11]); } while (0)

#endif
