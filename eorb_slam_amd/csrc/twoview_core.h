/* twoview_core.h -- the 3x3 algebra and the decision rules of TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:67-262,
 * ReconstructF :610-710 / :902-979, ReconstructH :712-873 / :991-1175, resolveReconstStat* :876-900 / :981-989, DecomposeE :1354-1375,
 * the head of CheckRT :1258-1270) in one text for both sides, after the pattern of mlpnp_core.h: twoview.hip includes it for the device,
 * tests/twoview_ref/reconstruct_ref.c for the CPU restatement.  C / C++ common subset, strict IEEE (-ffp-contract=off on both sides).
 * What the two sides write separately is everything with a shape: the RANSAC, CheckRT, the count of the inliers, the copies into the
 * result slots.  The second, independent writing of the rules and of the hypotheses is tests/twoview_ref/reconstruct_model.py.
 * The OpenCV 3.4.1 calls are restated on their scalar paths from knowledge of the published code; DESIGN.md section 2, "Parity choices of
 * the two-view reconstruction", has one paragraph per reading.  None is pinned against a build of the reference.
 *
 * The includer defines, before the include:
 *   TVC_FN                       the function qualifier
 *   TVC_HI(x) TVC_LO(x)          the high / low word of a double as int32_t / uint32_t;  TVC_MK(hi, lo) the double of two words
 *   TVC_SVD33(A, w, u, vt)       cv::SVD::compute of a 3x3 float matrix (row-major), with or without FULL_UV: the two are one
 *                                computation on a square matrix
 *   TVC_UNROLL                   a loop-unrolling pragma, or nothing
 * and includes eorb_fe.h (eorb_tvr_recon_params, eorb_tvr_recon_result, EORB_TVR_FORM_*).
 */
#ifndef TWOVIEW_CORE_H
#define TWOVIEW_CORE_H

/* ---- fdlibm e_acos.c, the whole domain (cosParallax can be negative; mlpnp_core.h's dev_dacos is stated for x >= 0 only) -------------- */
TVC_FN double tvc_dacos(double x)
{
    const double one = 1.0, pi = 3.14159265358979311600e+00, pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const int32_t hx = TVC_HI(x), ix = hx & 0x7fffffff;
    double z, p, q, r, w, s, c, df;
    if (ix >= 0x3ff00000) {                                  /* |x| >= 1 */
        if ((((uint32_t)ix - 0x3ff00000u) | TVC_LO(x)) == 0) /* |x| == 1 */
            return hx > 0 ? 0.0 : pi + 2.0 * pio2_lo;
        return (x - x) / (x - x);                            /* acos(|x| > 1) is NaN */
    }
    if (ix < 0x3fe00000) {                                   /* |x| < 0.5 */
        if (ix <= 0x3c600000) return pio2_hi + pio2_lo;      /* |x| < 2**-57 */
        z = x * x;
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        r = p / q;
        return pio2_hi - (x - (pio2_lo - r * x));
    }
    if (hx < 0) {                                            /* x < -0.5 */
        z = (one + x) * 0.5;
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        s = sqrt(z);
        r = p / q;
        w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    z = (one - x) * 0.5;                                     /* x > 0.5 */
    s = sqrt(z);
    df = TVC_MK(TVC_HI(s), 0u);
    c = (z - df * df) / (s + df);
    p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    r = p / q;
    w = r * s + c;
    return 2.0 * (df + w);
}

/* CheckRT :1341-1349: parallax = static_cast<float>(acos(vCosParallax[idx])*180/CV_PI), 0 when nGood == 0 */
TVC_FN float tvc_parallax(int n_good, float cos_sel)
{
    if (!(n_good > 0)) return 0.f;
    return (float)(tvc_dacos((double)cos_sel) * 180 / 3.1415926535897932384626433832795);
}

/* ---- OpenCV 3.4.1 primitives, scalar paths ------------------------------------------------------------------------------------------ */
/* cv::gemm, the small-matrix branch (flags == 0, len == 3, no C): three float products summed in float, then (float)(t*alpha + c*beta)
 * in double with c*beta = 0*0.  d may be a or b. */
TVC_FN void tvc_gemm33(const float* a, const float* b, double alpha, float* d)
{
    float r[9];
    int i, j;
    TVC_UNROLL
    for (i = 0; i < 3; i++)
        TVC_UNROLL
        for (j = 0; j < 3; j++) {
            const float t = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
            r[3 * i + j] = (float)((double)t * alpha + 0.0 * 0.0);
        }
    TVC_UNROLL
    for (i = 0; i < 9; i++) d[i] = r[i];
}
/* the same branch with one column: d = a*x */
TVC_FN void tvc_gemm3x1(const float* a, const float* x, float* d)
{
    float r[3];
    int i;
    TVC_UNROLL
    for (i = 0; i < 3; i++) {
        const float t = a[3 * i] * x[0] + a[3 * i + 1] * x[1] + a[3 * i + 2] * x[2];
        r[i] = (float)((double)t * 1.0 + 0.0 * 0.0);
    }
    TVC_UNROLL
    for (i = 0; i < 3; i++) d[i] = r[i];
}
/* cv::gemm with GEMM_1_T / GEMM_2_T: a transposed flag rules the small-matrix branch out (it requires flags == 0); GEMMSingleMul<float,
 * double> multiplies and sums in double, in the order of the inner index, and stores (float)(s*alpha).  at: d = a^T * b;  bt: d = a * b^T;
 * b has `cols` columns (3, or 1 for a vector) */
TVC_FN void tvc_gemm_at(const float* a, const float* b, int cols, double alpha, float* d)
{
    float r[9];
    int i, j, k;
    TVC_UNROLL
    for (i = 0; i < 3; i++)
        for (j = 0; j < cols; j++) {
            double s = 0;
            TVC_UNROLL
            for (k = 0; k < 3; k++) s += (double)a[3 * k + i] * (double)b[cols * k + j];
            r[cols * i + j] = (float)(s * alpha);
        }
    for (i = 0; i < 3 * cols; i++) d[i] = r[i];
}
TVC_FN void tvc_gemm33_bt(const float* a, const float* b, float* d)
{
    float r[9];
    int i, j, k;
    TVC_UNROLL
    for (i = 0; i < 3; i++)
        TVC_UNROLL
        for (j = 0; j < 3; j++) {
            double s = 0;
            TVC_UNROLL
            for (k = 0; k < 3; k++) s += (double)a[3 * i + k] * (double)b[3 * j + k];
            r[3 * i + j] = (float)(s * 1.0);
        }
    TVC_UNROLL
    for (i = 0; i < 9; i++) d[i] = r[i];
}
/* a MatExpr scale (Mat / double, Mat *= double, -Mat) assigned through convertTo: a copy when |alpha - 1| < DBL_EPSILON (noScale), else
 * cvtScale32f: src*(float)alpha + 0.0f.  "/ s" arrives here as alpha = 1./s, "-m" as alpha = -1 (so a zero comes out as +0). */
TVC_FN void tvc_scale(int n, const float* src, double alpha, float* dst)
{
    const int copy = fabs(alpha - 1) < 2.2204460492503131e-16;
    const float a = (float)alpha;
    int i;
    for (i = 0; i < n; i++) dst[i] = copy ? src[i] : src[i] * a + 0.0f;
}
/* cv::determinant, 3x3 CV_32F: the det3 macro, the 2x2 minors in double */
TVC_FN double tvc_det3(const float* m)
{
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}
/* cv::norm(NORM_L2) of a continuous 3x1 float Mat: normL2Sqr<float, double>, std::sqrt */
TVC_FN double tvc_norm3(const float* a)
{
    double s = 0, result;
    int i;
    TVC_UNROLL
    for (i = 0; i < 3; i++) { const double v = a[i]; s += v * v; }
    result = 0 + s;
    return sqrt(result);
}
/* Mat::inv() 3x3: cv::invert, DECOMP_LU, the n == 3 closed form (determinant and cofactors in double, d = 1./d; d == 0 gives zeros) */
TVC_FN void tvc_inv33(const float* S, float* D)
{
#define TVC_S(r, c) S[3 * (r) + (c)]
    double d = tvc_det3(S);
    int i;
    if (d != 0.) {
        double t[9];
        d = 1. / d;
        t[0] = ((double)TVC_S(1, 1) * TVC_S(2, 2) - (double)TVC_S(1, 2) * TVC_S(2, 1)) * d;
        t[1] = ((double)TVC_S(0, 2) * TVC_S(2, 1) - (double)TVC_S(0, 1) * TVC_S(2, 2)) * d;
        t[2] = ((double)TVC_S(0, 1) * TVC_S(1, 2) - (double)TVC_S(0, 2) * TVC_S(1, 1)) * d;
        t[3] = ((double)TVC_S(1, 2) * TVC_S(2, 0) - (double)TVC_S(1, 0) * TVC_S(2, 2)) * d;
        t[4] = ((double)TVC_S(0, 0) * TVC_S(2, 2) - (double)TVC_S(0, 2) * TVC_S(2, 0)) * d;
        t[5] = ((double)TVC_S(0, 2) * TVC_S(1, 0) - (double)TVC_S(0, 0) * TVC_S(1, 2)) * d;
        t[6] = ((double)TVC_S(1, 0) * TVC_S(2, 1) - (double)TVC_S(1, 1) * TVC_S(2, 0)) * d;
        t[7] = ((double)TVC_S(0, 1) * TVC_S(2, 0) - (double)TVC_S(0, 0) * TVC_S(2, 1)) * d;
        t[8] = ((double)TVC_S(0, 0) * TVC_S(1, 1) - (double)TVC_S(0, 1) * TVC_S(1, 0)) * d;
        TVC_UNROLL
        for (i = 0; i < 9; i++) D[i] = (float)t[i];
    } else {
        TVC_UNROLL
        for (i = 0; i < 9; i++) D[i] = 0.f;
    }
#undef TVC_S
}

/* ---- one hypothesis as CheckRT takes it: pose = R[9] t[3] P2[12] O2[3] (eorb_tvr_pose) ------------------------------------------------
 * P2 = K*[R|t] (:1265-1268): gemm, flags == 0, len == 3 == the height of the 3x4 result: the small-matrix branch, column by column.
 * O2 = -R.t()*t (:1270): MatOp_T with alpha = -1, then one gemm(R, t, -1, GEMM_1_T). */
TVC_FN void tvc_pose(const float* K, const float* R, const float* t, float* pose)
{
    int i, j;
    TVC_UNROLL
    for (i = 0; i < 9; i++) pose[i] = R[i];
    TVC_UNROLL
    for (i = 0; i < 3; i++) pose[9 + i] = t[i];
    TVC_UNROLL
    for (i = 0; i < 3; i++)
        TVC_UNROLL
        for (j = 0; j < 4; j++) {
            const float b0 = j < 3 ? R[j] : t[0], b1 = j < 3 ? R[3 + j] : t[1], b2 = j < 3 ? R[6 + j] : t[2];
            const float s = K[3 * i] * b0 + K[3 * i + 1] * b1 + K[3 * i + 2] * b2;
            pose[12 + 4 * i + j] = (float)((double)s * 1.0 + 0.0 * 0.0);
        }
    tvc_gemm_at(R, t, 1, -1.0, pose + 24);
}

/* ReconstructF's hypotheses (:617-626 / :912-921): E21 = K.t()*F21*K, DecomposeE, t1 = t, t2 = -t; poses[4] in the order R1t1, R2t1,
 * R1t2, R2t2 */
TVC_FN void tvc_hypotheses_f(const float* K, const float* F21, float* poses)
{
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float KtF[9], E[9], w[3], u[9], vt[9], t[3], t1[3], t2[3], tmp[9], R1[9], R2[9];
    tvc_gemm_at(K, F21, 3, 1.0, KtF);                       /* K.t()*F21: GEMM_1_T */
    tvc_gemm33(KtF, K, 1.0, E);                             /* (...)*K: the temporary times K, flags == 0 */
    TVC_SVD33(E, w, u, vt);
    t[0] = u[2]; t[1] = u[5]; t[2] = u[8];                  /* u.col(2).copyTo(t) */
    tvc_scale(3, t, 1. / tvc_norm3(t), t1);                 /* t = t/cv::norm(t) */
    tvc_gemm33(u, W, 1.0, tmp); tvc_gemm33(tmp, vt, 1.0, R1);
    if (tvc_det3(R1) < 0) tvc_scale(9, R1, -1.0, R1);
    tvc_gemm33_bt(u, W, tmp); tvc_gemm33(tmp, vt, 1.0, R2); /* u*W.t(): GEMM_2_T */
    if (tvc_det3(R2) < 0) tvc_scale(9, R2, -1.0, R2);
    tvc_scale(3, t1, -1.0, t2);                             /* t2 = -t */
    tvc_pose(K, R1, t1, poses); tvc_pose(K, R2, t1, poses + 27); tvc_pose(K, R1, t2, poses + 54); tvc_pose(K, R2, t2, poses + 81);
}

/* ReconstructH's hypotheses (:719-825 / :1001-1107), Faugeras' decomposition; returns 0 when the d1/d2, d2/d3 test leaves (nothing is
 * written), else 1 with poses[8] = vR[0..7], vt[0..7].  The normals vn are computed by the reference and never read: not here. */
TVC_FN int tvc_hypotheses_h(const float* K, const float* H21, float thRDH, float* poses)
{
    float invK[9], tmp[9], A[9], w[3], U[9], Vt[9], Rp[9], R[9], tp[3], t[3], tn[3];
    float x1[4], x3[4], stheta[4], sphi[4];
    int i;
    tvc_inv33(K, invK);
    tvc_gemm33(invK, H21, 1.0, tmp); tvc_gemm33(tmp, K, 1.0, A);
    TVC_SVD33(A, w, U, Vt);
    {
        const float s = (float)(tvc_det3(U) * tvc_det3(Vt));
        const float d1 = w[0], d2 = w[1], d3 = w[2];
        if (d1 / d2 < thRDH || d2 / d3 < thRDH) return 0;
        {
            const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
            const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
            const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
            const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
            const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
            const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
            x1[0] = aux1; x1[1] = aux1; x1[2] = -aux1; x1[3] = -aux1;
            x3[0] = aux3; x3[1] = -aux3; x3[2] = aux3; x3[3] = -aux3;
            stheta[0] = aux_stheta; stheta[1] = -aux_stheta; stheta[2] = -aux_stheta; stheta[3] = aux_stheta;
            sphi[0] = aux_sphi; sphi[1] = -aux_sphi; sphi[2] = -aux_sphi; sphi[3] = aux_sphi;
            for (i = 0; i < 8; i++) {
                const int k = i & 3;
                Rp[1] = 0.f; Rp[3] = 0.f; Rp[5] = 0.f; Rp[7] = 0.f;
                if (i < 4) {                                /* case d' = d2 */
                    Rp[0] = ctheta; Rp[2] = -stheta[k]; Rp[4] = 1.f; Rp[6] = stheta[k]; Rp[8] = ctheta;
                    tp[0] = x1[k]; tp[1] = 0.f; tp[2] = -x3[k];
                    tvc_scale(3, tp, (double)(d1 - d3), tp);                /* tp *= d1-d3 */
                } else {                                    /* case d' = -d2 */
                    Rp[0] = cphi; Rp[2] = sphi[k]; Rp[4] = -1.f; Rp[6] = sphi[k]; Rp[8] = -cphi;
                    tp[0] = x1[k]; tp[1] = 0.f; tp[2] = x3[k];
                    tvc_scale(3, tp, (double)(d1 + d3), tp);                /* tp *= d1+d3 */
                }
                tvc_gemm33(U, Rp, (double)s, tmp);          /* s*U*Rp*Vt: gemm(U, Rp, alpha = s), then the temporary times Vt */
                tvc_gemm33(tmp, Vt, 1.0, R);
                tvc_gemm3x1(U, tp, t);                      /* t = U*tp */
                tvc_scale(3, t, 1. / tvc_norm3(t), tn);     /* t/cv::norm(t) */
                tvc_pose(K, R, tn, poses + 27 * i);
            }
        }
    }
    return 1;
}

/* ---- the four decision rules -------------------------------------------------------------------------------------------------------------
 * On entry r->is_homography and r->n_hyp (4 or 8) are set; ng / par: nGood and parallax per hypothesis in hypothesis order; N: the inlier
 * count of ReconstructF / ReconstructH.  Fills ok, n_min_good, n_similar, hyp_good, hyp_parallax, info_good, hyp_best, hyp_second,
 * best_good, second_good, best_parallax, second_parallax.  The comparisons keep the reference's types. */
TVC_FN void tvc_resolve(const eorb_tvr_recon_params* p, int N, const int32_t* ng, const float* par, eorb_tvr_recon_result* r)
{
    const int nh = r->n_hyp, info = p->form == EORB_TVR_FORM_INFO;
    const float minParallax = p->min_parallax;
    const int minTriangulated = p->min_triangulated;
    int i;
    for (i = 0; i < 8; i++) { r->hyp_good[i] = i < nh ? ng[i] : 0; r->hyp_parallax[i] = i < nh ? par[i] : 0.f; r->info_good[i] = 0; }
    r->ok = 0; r->n_min_good = 0; r->n_similar = 0; r->hyp_best = -1; r->hyp_second = -1;
    r->best_good = 0; r->second_good = 0; r->best_parallax = 0.f; r->second_parallax = 0.f;
    if (!r->is_homography && !info) {
        /* ReconstructF :638-709 */
        int maxGood = ng[0], nMinGood, nsimilar = 0, first = 0, reject;
        float thMaxGoodR = p->th_max_good_r_f;
        for (i = 1; i < 4; i++) if (ng[i] > maxGood) maxGood = ng[i];
        nMinGood = (int)(p->th_min_good_r * N);
        if (nMinGood < minTriangulated) nMinGood = minTriangulated;
        for (i = 0; i < 4; i++) if (ng[i] > thMaxGoodR * maxGood) nsimilar++;
        reject = maxGood < nMinGood || nsimilar > 1;
        for (i = 3; i >= 0; i--) if (maxGood == ng[i]) first = i;      /* the if / else-if chain: the first equal count */
        r->n_min_good = nMinGood; r->n_similar = nsimilar;
        r->best_good = maxGood; r->best_parallax = par[first];
        if (!reject && par[first] > minParallax) { r->ok = 1; r->hyp_best = first; }
    } else if (!r->is_homography) {
        /* ReconstructF :937-978: the multimap<int, ..., greater<int>>; an equal key goes in at the upper bound, after its equals */
        int order[4], n = 0, k, maxGood, nMinGood, nsimilar = 0, distinctTrans;
        float thMaxGoodR = p->th_max_good_r_f;
        for (i = 0; i < 4; i++) {
            int pos = n;
            while (pos > 0 && ng[order[pos - 1]] < ng[i]) pos--;
            for (k = n; k > pos; k--) order[k] = order[k - 1];
            order[pos] = i; n++;
        }
        for (i = 0; i < 4; i++) r->info_good[i] = ng[order[i]];
        r->hyp_best = order[0]; r->hyp_second = order[1];
        r->best_good = ng[order[0]]; r->best_parallax = par[order[0]];
        r->second_good = ng[order[1]]; r->second_parallax = par[order[1]];
        /* resolveReconstStatF :876-900, over all of mvnGood (entries 4 .. 7 are 0 here) */
        maxGood = r->best_good;
        nMinGood = (int)(p->th_min_good_r * N);
        if (nMinGood < minTriangulated) nMinGood = minTriangulated;
        for (i = 0; i < 8; i++) if ((float)r->info_good[i] > thMaxGoodR * (float)maxGood) nsimilar++;
        r->n_min_good = nMinGood; r->n_similar = (unsigned char)nsimilar;
        distinctTrans = !(maxGood < nMinGood || nsimilar > 1);
        r->ok = (r->best_parallax > minParallax) && distinctTrans;
    } else {
        /* ReconstructH :828-872 / :1110-1174: strict >, the earlier hypothesis keeps a tie */
        int bestGood = 0, secondBestGood = 0, bestIdx = -1, secondIdx = -1;
        float bestParallax = -1, secondBestParallax = -1;
        for (i = 0; i < 8; i++) {
            const int nGood = ng[i];
            if (nGood > bestGood) {
                secondBestGood = bestGood; bestGood = nGood;
                secondIdx = bestIdx; bestIdx = i;
                secondBestParallax = bestParallax; bestParallax = par[i];
            } else if (nGood > secondBestGood) {
                secondBestGood = nGood; secondIdx = i; secondBestParallax = par[i];
            }
            if (info) r->info_good[i] = nGood;
        }
        r->best_good = bestGood; r->second_good = secondBestGood; r->best_parallax = bestParallax;
        if (!info) {
            r->ok = secondBestGood < p->th_max_good_r_h * bestGood && bestParallax >= minParallax && bestGood > minTriangulated &&
                    bestGood > p->th_min_good_r * N;
            if (r->ok) r->hyp_best = bestIdx;
        } else {
            /* resolveReconstStatH :981-989 */
            const float fBest = (float)bestGood, fSecond = (float)secondBestGood;
            r->second_parallax = secondBestParallax;
            r->hyp_best = bestIdx; r->hyp_second = secondIdx;      /* -1 where the reference reads vR[-1] */
            r->ok = fSecond < p->th_max_good_r_h * fBest && bestParallax >= minParallax && bestGood > minTriangulated &&
                    fBest > p->th_min_good_r * (float)N;
        }
    }
}

#endif
