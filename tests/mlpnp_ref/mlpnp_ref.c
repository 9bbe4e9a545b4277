/*
 * mlpnp_ref.c -- TEST INFRASTRUCTURE: what eorb_mlpnp_ransac computes, stated sequentially in strict IEEE C (no FMA contraction) from
 * src/MLPnPsolver.cpp.  The scalar algebra (Eigen 3.3's algorithms on their scalar paths, fdlibm's acos / pow, the project's own
 * Jacobian) is eorb_slam_amd/csrc/mlpnp_core.h, the one text the device compiles too; tests/test_mlpnp_ref.py holds every piece of it to
 * plain float64 numpy models.  What is written here is what the device writes in its own way: the loops over correspondences, rows,
 * sets and iterations, and the result rule -- here in the order of the source, one iteration after the other.  None of the Eigen
 * readings is pinned against a build of the reference ("Parity choices of the MLPnP solver").
 * The camera projections are proj_ref.c's (Pinhole quotient form; KannalaBrandt8 through pr_set_project); unproject is the oracle's
 * orc_camera_unproject, handed in through mlr_set_unproject.
 */
#include "../proj_ref/proj_ref.c"
#include <float.h>
#include <stdlib.h>

/* ---- options and the branch probe ------------------------------------------------------------------------------------------------ */
enum { MLO_HOST_LIBM = 0, MLO_BOUND_LE, MLO_BEST_GE, MLO_REFINE_STORES, MLO_REFINE_GE, MLO_TRIGGER_GT, MLO_N };   /* libm's acos / pow; the named wrong variants */
static int g_opt[MLO_N];
void mlr_set_option(int which, int v) { if (which >= 0 && which < MLO_N) g_opt[which] = v; }

static long g_probe[64];
#define MLP_PROBE(id) (g_probe[id]++)

static double mk_double(uint32_t hi, uint32_t lo) { const uint64_t u = ((uint64_t)hi << 32) | lo; double d; memcpy(&d, &u, 8); return d; }
static int32_t hi_word(double x) { uint64_t u; memcpy(&u, &x, 8); return (int32_t)(u >> 32); }
static uint32_t lo_word(double x) { uint64_t u; memcpy(&u, &x, 8); return (uint32_t)u; }

/* ---- fdlibm k_sin / k_cos with the two-term pi/2 reduction, the text of dev_dsincos (|x| < 100; a NaN gives two NaNs) ------------------ */
static double ml_ksin(double x, double y, int iy)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x, v = z * x, r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (iy == 0) return x + v * (S1 + z * r);
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
static double ml_kcos(double x, double y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x, r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))))), ax = fabs(x);
    if (ax < 0.3) return 1.0 - (0.5 * z - (z * r - x * y));
    double qx = 0.28125;
    if (!(ax > 0.78125)) { const double q = 0.25 * ax; qx = mk_double((uint32_t)hi_word(q), 0u); }
    const double hz = 0.5 * z - qx, a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}
static void ml_dsincos(double x, double* sn, double* cs)
{
    if (x != x) { *sn = x; *cs = x; return; }
    if (fabs(x) <= 0.78539816339744830962) { *sn = ml_ksin(x, 0.0, 0); *cs = ml_kcos(x, 0.0); return; }
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11;
    const double t = fabs(x);
    int n = (int)(t * invpio2 + 0.5);
    const double fn = (double)n, r = t - fn * pio2_1, w = fn * pio2_1t;
    double a = r - w, b = (r - a) - w;
    if (x < 0) { a = -a; b = -b; n = -n; }
    const double ks = ml_ksin(a, b, 1), kc = ml_kcos(a, b);
    switch (n & 3) {
        case 0: *sn = ks; *cs = kc; break;
        case 1: *sn = kc; *cs = -ks; break;
        case 2: *sn = -ks; *cs = -kc; break;
        default: *sn = -kc; *cs = ks; break;
    }
}

#define MLP_FN static
#define MLP_SINCOS(x, ps, pc) ml_dsincos((x), (ps), (pc))
#define MLP_HI(x) hi_word(x)
#define MLP_LO(x) lo_word(x)
#define MLP_MK(hi, lo) mk_double((uint32_t)(hi), (uint32_t)(lo))
static double dev_dacos(double x);
static double dev_dpow(double x, double y);
#define MLP_ACOS(x) (g_opt[MLO_HOST_LIBM] ? acos(x) : dev_dacos(x))
#define MLP_CBRT(x) (g_opt[MLO_HOST_LIBM] ? pow((x), 1.0 / 3.0) : dev_dpow((x), 1.0 / 3.0))
#include "../../eorb_slam_amd/csrc/mlpnp_core.h"

void mlr_probe_reset(void) { memset(g_probe, 0, sizeof g_probe); }
void mlr_probe_read(long* out) { memcpy(out, g_probe, sizeof(long) * MLPP_N); }
int mlr_probe_count(void) { return MLPP_N; }

/* ---- the pieces, for tests/test_mlpnp_ref.py ---------------------------------------------------------------------------------------- */
void mlr_acos_n(const double* x, long n, double* out) { for (long i = 0; i < n; i++) out[i] = dev_dacos(x[i]); }
void mlr_host_acos_n(const double* x, long n, double* out) { for (long i = 0; i < n; i++) out[i] = acos(x[i]); }
void mlr_pow_n(const double* x, double y, long n, double* out) { for (long i = 0; i < n; i++) out[i] = dev_dpow(x[i], y); }
void mlr_host_pow_n(const double* x, double y, long n, double* out) { for (long i = 0; i < n; i++) out[i] = pow(x[i], y); }
void mlr_nullspace_n(const double* f, long n, double* ns) { for (long i = 0; i < n; i++) mlp_nullspace(f + 3 * i, ns + 6 * i); }
int mlr_jsvd(const double* A, int n, double* V, double* U, double* sv)
{
    double W[144];
    return mlp_jsvd(A, n, W, V, U, sv);
}
int mlr_rank3(const double* M) { double m[9]; memcpy(m, M, sizeof m); return mlp_rank3(m); }
void mlr_eig3(const double* M, double* w, double* Q) { double sub[2]; mlp_eig3(M, w, Q, sub); }
void mlr_ldlt_solve(const double* A, const double* g, double* dx) { double a[36], temp[6]; int tr[6]; memcpy(a, A, sizeof a); mlp_ldlt_solve(a, g, dx, tr, temp); }
/* residuals r[2] and Jacobian J[2][6] of one correspondence at x = (omega, T) */
void mlr_residual_jac(const double* x, const double* X, const double* ns, double* r, double* J)
{
    double R[9], B[9];
    mlp_gn_frame(x, R, B);
    mlp_gn_point(R, B, x + 3, X, ns, r, J);
}

/* ---- computePose (:395-701) of the correspondences idx[0..cnt): f[.][3], ns[.][6], X[.][3] per correspondence -> Rt[12] ------------- */
typedef struct { const double* f; const double* ns; const double* X; } ml_prep;
static void ml_compute_pose(const ml_prep* P, const int32_t* idx, int cnt, double* rows, double* Rt)
{
    double M[9], Mq[9], Q[9], eig[9], ew[3], sub[2], A[144], W[144], V[144], sv[12], res1[12], X6[18], f6[18];
    double x[6], R[9], B[9], A6[36], g[6], dx[6], temp[6], ws[64];
    int tr[6];
    for (int e = 0; e < 9; e++) {
        const int i = e / 3, j = e % 3;
        double s = 0.0;
        for (int k = 0; k < cnt; k++) { const double* X = P->X + 3 * (size_t)idx[k]; s += X[i] * X[j]; }
        M[e] = s;
    }
    memcpy(Mq, M, sizeof M);
    const int planar = mlp_rank3(Mq) == 2;
    for (int i = 0; i < 9; i++) eig[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (planar) {
        mlp_eig3(M, ew, Q, sub);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) eig[3 * i + j] = Q[3 * j + i];
    }
    for (int p = 0; p < 6; p++)
        for (int k = 0; k < 3; k++) { X6[3 * p + k] = P->X[3 * (size_t)idx[p] + k]; f6[3 * p + k] = P->f[3 * (size_t)idx[p] + k]; }
    const int n = planar ? 9 : 12;
    for (int ca = 0; ca < n; ca++)
        for (int cb = 0; cb < n; cb++) {
            double s = 0.0;
            for (int k = 0; k < cnt; k++) {
                const double* X = P->X + 3 * (size_t)idx[k];
                const double* ns = P->ns + 6 * (size_t)idx[k];
                double p0 = X[0], p1 = X[1], p2 = X[2];
                if (planar) {
                    p0 = eig[0] * X[0] + eig[1] * X[1] + eig[2] * X[2];
                    p1 = eig[3] * X[0] + eig[4] * X[1] + eig[5] * X[2];
                    p2 = eig[6] * X[0] + eig[7] * X[1] + eig[8] * X[2];
                }
                s += mlp_design(planar, ns, p0, p1, p2, 0, ca) * mlp_design(planar, ns, p0, p1, p2, 0, cb);
                s += mlp_design(planar, ns, p0, p1, p2, 1, ca) * mlp_design(planar, ns, p0, p1, p2, 1, cb);
            }
            A[ca * n + cb] = s;
        }
    mlp_jsvd(A, n, W, V, NULL, sv);
    for (int i = 0; i < n; i++) res1[i] = V[i * n + n - 1];
    mlp_recover_pose(planar, res1, eig, X6, f6, x, ws);
    int it_cnt = 0, by_break = 0;
    while (it_cnt < 5) {
        mlp_gn_frame(x, R, B);
        for (int k = 0; k < cnt; k++) {
            double* row = rows + 14 * (size_t)k;
            mlp_gn_point(R, B, x + 3, P->X + 3 * (size_t)idx[k], P->ns + 6 * (size_t)idx[k], row + 12, row);
        }
        for (int i = 0; i < 6; i++) {
            for (int j = 0; j < 6; j++) {
                double s = 0.0;
                for (int k = 0; k < cnt; k++) { const double* row = rows + 14 * (size_t)k; s += row[i] * row[j]; s += row[6 + i] * row[6 + j]; }
                A6[6 * i + j] = s;
            }
            double s = 0.0;
            for (int k = 0; k < cnt; k++) { const double* row = rows + 14 * (size_t)k; s += row[i] * row[12]; s += row[6 + i] * row[13]; }
            g[i] = s;
        }
        mlp_ldlt_solve(A6, g, dx, tr, temp);
        if (mlp_gn_dx_guard(dx)) { MLP_PROBE(MLPP_GN_EXIT_DX); by_break = 1; break; }
        /* maxCoeff of |Jac*dx|: entry 0 first, replaced on > */
        double mx = 0.0;
        for (int k = 0; k < cnt; k++)
            for (int r = 0; r < 2; r++) {
                const double* row = rows + 14 * (size_t)k + 6 * r;
                double dl = 0.0;
                for (int i = 0; i < 6; i++) dl += row[i] * dx[i];
                dl = fabs(dl);
                if (k == 0 && r == 0) mx = dl;
                else if (dl > mx) mx = dl;
            }
        for (int i = 0; i < 6; i++) x[i] = x[i] - dx[i];
        if (mx < 1e-5) { MLP_PROBE(MLPP_GN_EXIT_DL); by_break = 1; break; }
        it_cnt++;
    }
    if (!by_break) MLP_PROBE(MLPP_GN_EXIT_MAXIT);
    mlp_rodrigues2rot(x, R);
    for (int i = 0; i < 9; i++) Rt[i] = R[i];
    for (int i = 0; i < 3; i++) Rt[9 + i] = x[3 + i];
}

typedef void (*ml_unproject_fn)(const pr_camera*, float, float, float*);
static ml_unproject_fn g_unproject = 0;
void mlr_set_unproject(ml_unproject_fn f) { g_unproject = f; }

/* the constructor's arithmetic (:73-88) and mvMaxError (:302) */
static void ml_prepare(const pr_camera* cam, int N, const float* p2d, const float* Xw, const float* sigma2, float th2,
                       double* f, double* ns, double* X, float* bound)
{
    MLP_PROBE(cam->model ? MLPP_KB8 : MLPP_PINHOLE);
    for (int i = 0; i < N; i++) {
        float br[3];
        g_unproject(cam, p2d[2 * i], p2d[2 * i + 1], br);
        const float z = br[2];
        br[0] /= z; br[1] /= z; br[2] /= z;
        for (int k = 0; k < 3; k++) { f[3 * i + k] = (double)br[k]; X[3 * i + k] = (double)Xw[3 * i + k]; }
        mlp_nullspace(f + 3 * i, ns + 6 * i);
        bound[i] = sigma2[i] * th2;
    }
}
static int ml_is_inlier(const pr_camera* cam, const double* Rt, const float* X, const float* p, float bound)
{
    float xc[3], u, v;
    MLP_CAMERA_POINT(Rt, X, xc);
    project(cam, xc, &u, &v);
    const float distX = p[0] - u, distY = p[1] - v;
    const float error2 = distX * distX + distY * distY;
    return g_opt[MLO_BOUND_LE] ? error2 <= bound : error2 < bound;
}
static int ml_check_inliers(const pr_camera* cam, const double* Rt, int N, const float* Xw, const float* p2d, const float* bound, uint8_t* flags)
{
    int n = 0;
    for (int i = 0; i < N; i++) { flags[i] = (uint8_t)ml_is_inlier(cam, Rt, Xw + 3 * i, p2d + 2 * i, bound[i]); n += flags[i]; }
    return n;
}
/* the strict < of :326 on a planted error */
int mlr_bound_test(float error2, float sigma2, float th2) { const float b = sigma2 * th2; return g_opt[MLO_BOUND_LE] ? error2 <= b : error2 < b; }

/* computePose of a planted problem for the tests: bearing vectors f[n][3] given as doubles, points X[n][3] -> Rt[12] */
void mlr_compute_pose(const double* f, const double* X, int n, double* Rt)
{
    double* ns = (double*)malloc(sizeof(double) * 6 * (size_t)n);
    double* rows = (double*)malloc(sizeof(double) * 14 * (size_t)n);
    int32_t* idx = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
    for (int i = 0; i < n; i++) { idx[i] = i; mlp_nullspace(f + 3 * i, ns + 6 * i); }
    const ml_prep P = {f, ns, X};
    ml_compute_pose(&P, idx, n, rows, Rt);
    free(ns); free(rows); free(idx);
}

typedef struct { int32_t N, iters, min_inliers; float th2; pr_camera cam; int32_t first_it, best_it; } ml_problem;      /* = eorb_mlpnp_problem */
typedef struct { int32_t stop_it, iterations_used, best_it, n_best, refined, n_inliers; float Tcw[16]; } ml_result;       /* = eorb_mlpnp_result */

static void ml_tcw(const double* Rt, float* T)
{
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[4 * r + c] = (float)Rt[3 * r + c]; T[4 * r + 3] = (float)Rt[9 + r]; }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

/* MLPnPsolver::iterate (:149-266) run to its end; the signature of eorb_mlpnp_ransac, then stop_early: 1 = compute no hypothesis
 * after the one Refine succeeded at, as the reference does (the timing baseline; the same results, the later aids stay zero) */
int mlr_ransac(const ml_problem* problems, int K, const float* p2d_all, const float* Xw_all, const float* sigma2_all, const int32_t* sets_all,
               ml_result* results, uint8_t* inliers_all, int32_t* it_inliers_all, double* it_Rt_all, int32_t* it_refine_all, int stop_early)
{
    size_t n0 = 0, i0 = 0;
    for (int kp = 0; kp < K; kp++) {
        const ml_problem* P = problems + kp;
        const int N = P->N, iters = P->iters;
        const float* p2d = p2d_all + 2 * n0; const float* Xw = Xw_all + 3 * n0; const float* sigma2 = sigma2_all + n0;
        const int32_t* sets = sets_all + 6 * i0;
        uint8_t* inliers = inliers_all + n0;
        ml_result* res = results + kp;
        memset(res, 0, sizeof *res);
        memset(inliers, 0, (size_t)N);
        if (it_inliers_all) memset(it_inliers_all + i0, 0, sizeof(int32_t) * (size_t)iters);
        if (it_Rt_all) memset(it_Rt_all + 12 * i0, 0, sizeof(double) * 12 * (size_t)iters);
        if (it_refine_all) for (int i = 0; i < iters; i++) it_refine_all[i0 + i] = -1;
        n0 += (size_t)N; i0 += (size_t)iters;
        if (N < P->min_inliers) { MLP_PROBE(MLPP_TOO_FEW); res->stop_it = -1; res->best_it = -1; continue; }
        double* f = (double*)malloc(sizeof(double) * 3 * (size_t)N); double* ns = (double*)malloc(sizeof(double) * 6 * (size_t)N);
        double* X = (double*)malloc(sizeof(double) * 3 * (size_t)N); float* bound = (float*)malloc(sizeof(float) * (size_t)N);
        double* rows = (double*)malloc(sizeof(double) * 14 * (size_t)N); int32_t* list = (int32_t*)malloc(sizeof(int32_t) * (size_t)N);
        uint8_t* flags = (uint8_t*)malloc((size_t)N); uint8_t* best_flags = (uint8_t*)calloc((size_t)N, 1); uint8_t* ref_flags = (uint8_t*)malloc((size_t)N);
        double* Rts = (double*)calloc(12 * (size_t)iters, sizeof(double)); int32_t* cnts = (int32_t*)calloc((size_t)iters, sizeof(int32_t));
        ml_prepare(&P->cam, N, p2d, Xw, sigma2, P->th2, f, ns, X, bound);
        const ml_prep prep = {f, ns, X};
        const size_t off = i0 - (size_t)iters;
        int bi = -1, bn = 0, stop = -1, refn = 0;
        double Rt_ref[12], Rt_dead[12];
        float Tbest[16];
        memset(Tbest, 0, sizeof Tbest);
        if (P->best_it >= 0) {      /* the running best carried in: its hypothesis and flags again */
            ml_compute_pose(&prep, sets + 6 * P->best_it, 6, rows, Rts + 12 * P->best_it);
            cnts[P->best_it] = ml_check_inliers(&P->cam, Rts + 12 * P->best_it, N, Xw, p2d, bound, flags);
            if (cnts[P->best_it] >= P->min_inliers) { bi = P->best_it; bn = cnts[bi]; memcpy(best_flags, flags, (size_t)N); ml_tcw(Rts + 12 * bi, Tbest); }
        }
        for (int pass = stop_early ? 1 : 0; pass < 2; pass++)
            for (int it = P->first_it; it < iters; it++) {
                if (pass == 0 || stop_early) {      /* computePose and CheckInliers of this set (:168-215) */
                    ml_compute_pose(&prep, sets + 6 * it, 6, rows, Rts + 12 * it);
                    cnts[it] = ml_check_inliers(&P->cam, Rts + 12 * it, N, Xw, p2d, bound, flags);
                    if (pass == 0) continue;
                } else ml_check_inliers(&P->cam, Rts + 12 * it, N, Xw, p2d, bound, flags);
                const int n = cnts[it];
                if (g_opt[MLO_TRIGGER_GT] ? n > P->min_inliers : n >= P->min_inliers) {
                    if (g_opt[MLO_BEST_GE] ? n >= bn : n > bn) { memcpy(best_flags, flags, (size_t)N); bn = n; bi = it; ml_tcw(Rts + 12 * it, Tbest); }
                    /* Refine (:338-392): computePose on the running best's inliers goes into a local `result` that is never stored
                     * (:367-371), so CheckInliers (:374) counts this iteration's mRi / mti again and mRefinedTcw / mvbRefinedInliers
                     * are this iteration's.  The dead computePose is kept here because the reference spends its time (the latency
                     * baseline); MLO_REFINE_STORES is the named wrong variant in which Refine would store what it computed. */
                    int m = 0;
                    for (int i = 0; i < N; i++) if (best_flags[i]) list[m++] = i;
                    ml_compute_pose(&prep, list, m, rows, Rt_dead);
                    const double* Rt_now = g_opt[MLO_REFINE_STORES] ? Rt_dead : Rts + 12 * it;
                    refn = ml_check_inliers(&P->cam, Rt_now, N, Xw, p2d, bound, ref_flags);
                    memcpy(Rt_ref, Rt_now, sizeof Rt_ref);
                    if (it_refine_all) it_refine_all[off + it] = refn;
                    if (g_opt[MLO_REFINE_GE] ? refn >= P->min_inliers : refn > P->min_inliers) { stop = it; break; }
                }
            }
        res->stop_it = stop; res->iterations_used = stop >= 0 ? stop + 1 : iters; res->best_it = bi; res->n_best = bn; res->refined = stop >= 0;
        if (stop >= 0) { MLP_PROBE(MLPP_REFINED); res->n_inliers = refn; ml_tcw(Rt_ref, res->Tcw); memcpy(inliers, ref_flags, (size_t)N); }
        else if (bn >= P->min_inliers) { MLP_PROBE(MLPP_BEST_RETURNED); res->n_inliers = bn; memcpy(res->Tcw, Tbest, sizeof Tbest); memcpy(inliers, best_flags, (size_t)N); }
        else MLP_PROBE(MLPP_NOTHING_RETURNED);
        if (it_inliers_all) memcpy(it_inliers_all + off, cnts, sizeof(int32_t) * (size_t)iters);
        if (it_Rt_all) memcpy(it_Rt_all + 12 * off, Rts, sizeof(double) * 12 * (size_t)iters);
        free(f); free(ns); free(X); free(bound); free(rows); free(list); free(flags); free(best_flags); free(ref_flags); free(Rts); free(cnts);
    }
    return 0;
}

/* the pose Refine computes from the flags of the pose Rt and never stores (:338-371), and the count it would have if it were stored: what
 * the named wrong variant MLO_REFINE_STORES returns; Rt_out[12] (optional) = that pose */
int mlr_refine_from(const ml_problem* P, const float* p2d, const float* Xw, const float* sigma2, const double* Rt, double* Rt_out)
{
    const int N = P->N;
    double* f = (double*)malloc(sizeof(double) * 3 * (size_t)N); double* ns = (double*)malloc(sizeof(double) * 6 * (size_t)N);
    double* X = (double*)malloc(sizeof(double) * 3 * (size_t)N); float* bound = (float*)malloc(sizeof(float) * (size_t)N);
    double* rows = (double*)malloc(sizeof(double) * 14 * (size_t)N); int32_t* list = (int32_t*)malloc(sizeof(int32_t) * (size_t)N);
    uint8_t* flags = (uint8_t*)malloc((size_t)N);
    ml_prepare(&P->cam, N, p2d, Xw, sigma2, P->th2, f, ns, X, bound);
    const ml_prep prep = {f, ns, X};
    ml_check_inliers(&P->cam, Rt, N, Xw, p2d, bound, flags);
    int m = 0, out = -1;
    double R2[12];
    for (int i = 0; i < N; i++) if (flags[i]) list[m++] = i;
    if (m >= 6) {
        ml_compute_pose(&prep, list, m, rows, R2);
        out = ml_check_inliers(&P->cam, R2, N, Xw, p2d, bound, flags);
        if (Rt_out) memcpy(Rt_out, R2, sizeof R2);
    }
    free(f); free(ns); free(X); free(bound); free(rows); free(list); free(flags);
    return out;
}
