// mlpnp.hip -- MLPnPsolver on gfx950: computePose (src/MLPnPsolver.cpp:395-701) with its Gauss-Newton refinement (:737-851) for every
// RANSAC set of K independent problems, CheckInliers (:305-336) for every hypothesis, and the walk of iterate (:163-265) with what Refine
// (:338-392) returns.  The scalar algebra (Eigen 3.3's JacobiSVD, FullPivHouseholderQR, SelfAdjointEigenSolver, LDLT on their scalar paths, the
// project's own Jacobian) is mlpnp_core.h, one text with the CPU restatement tests/mlpnp_ref/mlpnp_ref.c; what is written here is the
// shape: which lane owns which entry, the order of the sums over rows, the result rule.  -ffp-contract=off; DESIGN.md section 2.
//
// eorb_mlpnp_ransac is three launches:
//   pnp_prepare_kernel  one thread per correspondence: the bearing vector (:80-82), its two nullspace columns (a pure function of it, so
//                       once and not per hypothesis), the point as doubles, mvMaxError (:302)
//   pnp_hyp_kernel      one wavefront per (problem, iteration): pnp_compute_pose on the six points of the set, then CheckInliers over
//                       all correspondences, 64 at a time, counted by ballot
//   pnp_finish_kernel   one workgroup per problem: the walk over the counts (the running best, the first count above min_inliers, where
//                       Refine returns true), the result record and the winner's flags
// pnp_compute_pose is a wavefront's work.  The work matrix and V of the 12x12 (9x9 when planar) two-sided Jacobi SVD sit in LDS; the
// (p, q) sweep is serial as the algorithm has it; every lane derives the 2x2 rotation from the same LDS words, so from the same bits,
// and lane i applies it to column i (left) and row i (right, and V).  The sums over correspondences (points3*points3^T, A^T A, J^T J,
// J^T r) have one lane per matrix entry and are serial over the rows, because their order is part of the result; the maxima are
// order-free.  What is left (rank, the 3x3 eigen-solver and SVD, the pose choice, the 6x6 LDLT) runs on lane 0 in LDS.
#include "mlpnp.h"

namespace eorb {

#define MLP_FN __device__ __forceinline__
#define MLP_SINCOS(x, ps, pc) dev_dsincos_nan((x), (ps), (pc))      // |x| < 100: see mlp_rodrigues2rot
#define MLP_HI(x) ((int32_t)__double2hiint(x))
#define MLP_LO(x) ((uint32_t)__double2loint(x))
#define MLP_MK(hi, lo) __hiloint2double((int)(hi), (int)(lo))
#include "mlpnp_core.h"

struct PnpLds {
    double W[144], V[144], sv[12], res1[12];
    double M[9], Mq[9], Q[9], eig[9], ew[3], sub[2];
    double X6[18], f6[18];
    double x[6], R[9], B[9], A6[36], g[6], dx[6], temp[6], Rt[12];
    double ws[64];
    double rows6[6 * kPnpRowDoubles];
    double scale;
    unsigned long long dl_max;
    int tr[6];
    int planar, brk, stop, first_nan;
};

// computePose of the cnt correspondences idx[0..cnt) of problem P (the six of a set) by the whole workgroup -> L.Rt (R row-major, then t).
// rows: cnt * kPnpRowDoubles doubles of work space.  Every branch below is taken from LDS words, so by all lanes alike.
__device__ __forceinline__ void pnp_compute_pose(const PnpArgs& a, const PnpProb& P, const int32_t* idx, int cnt, PnpLds& L, double* rows)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t g0 = (size_t)P.corr_off;
    // 1. planarTest = points3 * points3^T
    if (tid < 9) {
        const int i = tid / 3, j = tid % 3;
        double s = 0.0;
        for (int k = 0; k < cnt; k++) { const double* X = a.X + 3 * (g0 + idx[k]); s += X[i] * X[j]; }
        L.M[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 0; i < 9; i++) L.Mq[i] = L.M[i];
        const int planar = mlp_rank3(L.Mq) == 2;
        L.planar = planar;
        if (planar) {
            mlp_eig3(L.M, L.ew, L.Q, L.sub);
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) L.eig[3 * i + j] = L.Q[3 * j + i];      // eigenRot, transposed in place (:436-437)
        } else {
            for (int i = 0; i < 9; i++) L.eig[i] = (i % 4 == 0) ? 1.0 : 0.0;
        }
        for (int p = 0; p < 6; p++)
            for (int k = 0; k < 3; k++) { L.X6[3 * p + k] = a.X[3 * (g0 + idx[p]) + k]; L.f6[3 * p + k] = a.f[3 * (g0 + idx[p]) + k]; }
    }
    __syncthreads();
    const int planar = L.planar, n = planar ? 9 : 12;
    // 3./4. A^T A, one lane per entry, serial over the 2*cnt rows
    for (int e = tid; e < n * n; e += nt) {
        const int ca = e / n, cb = e % n;
        double s = 0.0;
        for (int k = 0; k < cnt; k++) {
            const size_t g = g0 + idx[k];
            const double* X = a.X + 3 * g;
            const double* ns = a.ns + 6 * g;
            double pt[3] = {X[0], X[1], X[2]};
            if (planar) {
#pragma unroll
                for (int r = 0; r < 3; r++) pt[r] = L.eig[3 * r] * X[0] + L.eig[3 * r + 1] * X[1] + L.eig[3 * r + 2] * X[2];
            }
            s += mlp_design(planar, ns, pt[0], pt[1], pt[2], 0, ca) * mlp_design(planar, ns, pt[0], pt[1], pt[2], 0, cb);
            s += mlp_design(planar, ns, pt[0], pt[1], pt[2], 1, ca) * mlp_design(planar, ns, pt[0], pt[1], pt[2], 1, cb);
        }
        L.W[e] = s;
    }
    __syncthreads();
    if (tid == 0) L.scale = mlp_svd_scale(L.W, n);
    __syncthreads();
    const double scale = L.scale;
    for (int e = tid; e < n * n; e += nt) { L.W[e] = L.W[e] / scale; L.V[e] = (e % (n + 1) == 0) ? 1.0 : 0.0; }
    __syncthreads();
    {   // JacobiSVD<MatrixXd>(AtA, ComputeFullV): the sweeps
        const double precision = 2.0 * MLP_DBL_EPS, considerAsZero = 2.0 * 4.9406564584124654e-324;
        double maxDiag = mlp_svd_maxdiag(L.W, n);
        bool finished = false;
        while (!finished) {
            finished = true;
            for (int p = 1; p < n; p++)
                for (int q = 0; q < p; q++) {
                    const double thr0 = precision * maxDiag, threshold = considerAsZero > thr0 ? considerAsZero : thr0;
                    if (fabs(L.W[p * n + q]) > threshold || fabs(L.W[q * n + p]) > threshold) {
                        finished = false;
                        const mlp_rot2 r = mlp_svd2x2(L.W[p * n + p], L.W[p * n + q], L.W[q * n + p], L.W[q * n + q]);
                        __syncthreads();
                        if (tid < n) MLP_ROT_LEFT(L.W, n, p, q, tid, r.lc, r.ls);
                        __syncthreads();
                        if (tid < n) { MLP_ROT_RIGHT(L.W, n, p, q, tid, r.rc, r.rs); MLP_ROT_RIGHT(L.V, n, p, q, tid, r.rc, r.rs); }
                        __syncthreads();
                        const double da = fabs(L.W[p * n + p]), db = fabs(L.W[q * n + q]), ab = da > db ? da : db;
                        if (ab > maxDiag) maxDiag = ab;
                    }
                }
        }
    }
    __syncthreads();
    if (tid == 0) {
        mlp_svd_finish(L.W, L.V, nullptr, L.sv, n, scale);
        for (int i = 0; i < n; i++) L.res1[i] = L.V[i * n + n - 1];
        mlp_recover_pose(planar, L.res1, L.eig, L.X6, L.f6, L.x, L.ws);
    }
    __syncthreads();
    // 5. mlpnp_gn
    for (int it_cnt = 0; it_cnt < 5; it_cnt++) {
        if (tid == 0) { mlp_gn_frame(L.x, L.R, L.B); L.dl_max = 0ull; L.first_nan = 0; }
        __syncthreads();
        for (int k = tid; k < cnt; k += nt) {
            const size_t g = g0 + idx[k];
            double* row = rows + (size_t)kPnpRowDoubles * k;
            mlp_gn_point(L.R, L.B, L.x + 3, a.X + 3 * g, a.ns + 6 * g, row + 12, row);
        }
        __syncthreads();
        if (tid < 42) {      // J^T J (36 entries) and J^T r (6), serial over the rows
            const int i = tid < 36 ? tid / 6 : tid - 36, j = tid % 6;
            double s = 0.0;
            for (int k = 0; k < cnt; k++) {
                const double* row = rows + (size_t)kPnpRowDoubles * k;
                if (tid < 36) { s += row[i] * row[j]; s += row[6 + i] * row[6 + j]; }
                else { s += row[i] * row[12]; s += row[6 + i] * row[13]; }
            }
            if (tid < 36) L.A6[tid] = s; else L.g[i] = s;
        }
        __syncthreads();
        if (tid == 0) { mlp_ldlt_solve(L.A6, L.g, L.dx, L.tr, L.temp); L.brk = mlp_gn_dx_guard(L.dx); }
        __syncthreads();
        if (L.brk) break;
        // dl = Jac*dx; maxCoeff of |dl| visits entry 0 first and replaces on >: a NaN there stays, a NaN elsewhere is passed over
        for (int k = tid; k < cnt; k += nt) {
            const double* row = rows + (size_t)kPnpRowDoubles * k;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                double dl = 0.0;
#pragma unroll
                for (int i = 0; i < 6; i++) dl += row[6 * r + i] * L.dx[i];
                dl = fabs(dl);
                if (dl != dl) { if (k == 0 && r == 0) L.first_nan = 1; }
                else atomicMax(&L.dl_max, (unsigned long long)__double_as_longlong(dl));
            }
        }
        __syncthreads();
        if (tid == 0) {
            L.stop = !L.first_nan && __longlong_as_double((long long)L.dl_max) < 1e-5;
            for (int i = 0; i < 6; i++) L.x[i] = L.x[i] - L.dx[i];
        }
        __syncthreads();
        if (L.stop) break;
    }
    if (tid == 0) {
        mlp_rodrigues2rot(L.x, L.R);
        for (int i = 0; i < 9; i++) L.Rt[i] = L.R[i];
        for (int i = 0; i < 3; i++) L.Rt[9 + i] = L.x[3 + i];
    }
    __syncthreads();
}

// CheckInliers of correspondence g under Rt (:310-326); a NaN error fails its <
__device__ __forceinline__ bool pnp_is_inlier(const PnpArgs& a, const PnpProb& P, const double* Rt, size_t g)
{
    const float* X = a.Xw + 3 * g;
    float xc[3], u, v;
    MLP_CAMERA_POINT(Rt, X, xc);
    cam_project_f(P.cam, xc, u, v);
    const float distX = a.p2d[2 * g] - u, distY = a.p2d[2 * g + 1] - v;
    const float error2 = distX * distX + distY * distY;
    return error2 < a.bound[g];
}

__global__ __launch_bounds__(256) void pnp_prepare_kernel(PnpArgs a)
{
    const PnpProb& P = a.prob[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.N) return;
    const size_t g = (size_t)P.corr_off + i;
    float bx, by;
    cam_unproject(P.cam, a.p2d[2 * g], a.p2d[2 * g + 1], bx, by);
    // cv_br /= cv_br.z with z = 1: a float division by one
    const double f[3] = {(double)(bx / 1.f), (double)(by / 1.f), (double)(1.f / 1.f)};
    double ns[6];
    mlp_nullspace(f, ns);
#pragma unroll
    for (int k = 0; k < 3; k++) { a.f[3 * g + k] = f[k]; a.X[3 * g + k] = (double)a.Xw[3 * g + k]; }
#pragma unroll
    for (int k = 0; k < 6; k++) a.ns[6 * g + k] = ns[k];
    a.bound[g] = a.sigma2[g] * P.th2;
}

__global__ __launch_bounds__(64) void pnp_hyp_kernel(PnpArgs a)
{
    __shared__ PnpLds L;
    const PnpProb& P = a.prob[blockIdx.y];
    const int lane = threadIdx.x, it = blockIdx.x;
    if (it >= P.iters || ransac_skips(P) || (it < P.first_it && it != P.best_it)) return;
    const size_t h = (size_t)P.set_off + it;
    pnp_compute_pose(a, P, a.sets + 6 * h, 6, L, L.rows6);
    if (lane < 12) a.it_Rt[12 * h + lane] = L.Rt[lane];
    const int n = ransac_count_inliers(P.N, [&](int i) { return pnp_is_inlier(a, P, L.Rt, (size_t)P.corr_off + i); });
    if (lane == 0) a.it_inliers[h] = n;
}

// the walk of iterate (:163-265) over the counts, from first_it with the running best carried in.  Refine (:338-392) computes a pose from
// the running best's inliers into a local that it never stores (:367-371), so its CheckInliers (:374) counts the current hypothesis
// again: it returns true exactly when this iteration's count is > min_inliers, and mRefinedTcw / mvbRefinedInliers are this iteration's
// pose and flags.  The pose it computes has no effect on anything returned and is not computed here.
__global__ __launch_bounds__(256) void pnp_finish_kernel(PnpArgs a)
{
    const PnpProb& P = a.prob[blockIdx.x];
    const int tid = threadIdx.x;
    int32_t* res = a.res + kPnpResWords * blockIdx.x;
    int32_t* refine = a.it_refine + P.set_off;
    for (int it = tid; it < P.iters; it += 256) refine[it] = -1;
    if (ransac_skips(P)) { if (tid == 0) { res[0] = -1; res[2] = -1; } return; }      // (:154-158; everything else stays zero)
    __syncthreads();
    const int32_t* cnt = a.it_inliers + P.set_off;
    const size_t g0 = (size_t)P.corr_off;
    int bi = P.best_it, bn = bi >= 0 ? cnt[bi] : 0, stop = -1;
    if (bn < P.min_inliers) { bi = -1; bn = 0; }      // a carried iteration that never was a running best is none
    for (int it = P.first_it; it < P.iters && stop < 0; it++) {      // (every lane walks the same counts)
        const int n = cnt[it];
        if (n < P.min_inliers) continue;                              // (:217)
        if (n > bn) { bn = n; bi = it; }                              // (:220)
        if (tid == 0) refine[it] = n;                                 // Refine is invoked (:234): mnRefinedInliers = n
        if (n > P.min_inliers) stop = it;                             // (:379)
    }
    const bool refined = stop >= 0, have_best = !refined && bi >= 0;
    const int win = refined ? stop : bi;
    const double* Rtw = a.it_Rt + 12 * ((size_t)P.set_off + (win >= 0 ? win : 0));
    if (tid == 0) {
        res[0] = stop; res[1] = refined ? stop + 1 : P.iters; res[2] = bi; res[3] = bn; res[4] = refined;
        res[5] = refined ? cnt[stop] : have_best ? bn : 0;
    }
    if (!refined && !have_best) return;
    if (tid < 16) {      // Rcw / tcw converted to CV_32F into an identity (:225-231, :381-387)
        const int r = tid / 4, c = tid % 4;
        ((float*)res)[6 + tid] = r == 3 ? (c == 3 ? 1.f : 0.f) : (float)(c == 3 ? Rtw[9 + r] : Rtw[3 * r + c]);
    }
    for (int i = tid; i < P.N; i += 256) a.inliers[g0 + i] = pnp_is_inlier(a, P, Rtw, g0 + i) ? 1 : 0;      // the winner's flags again
}

int mlpnp_ransac_dev(eorb_ctx* c, const PnpArgs& a)
{
    { ProfScope ps(c, "pnp_prepare");
      pnp_prepare_kernel<<<dim3((a.max_N + 255) / 256, a.K), 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "pnp_prepare_kernel"); }
    { ProfScope ps(c, "pnp_hyp");
      pnp_hyp_kernel<<<dim3(a.max_iters, a.K), 64, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "pnp_hyp_kernel"); }
    { ProfScope ps(c, "pnp_finish");
      pnp_finish_kernel<<<a.K, 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "pnp_finish_kernel"); }
    return EORB_OK;
}

}  // namespace eorb
