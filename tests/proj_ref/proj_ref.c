/* proj_ref.c -- CPU restatement of the map-point projector (eorb_slam_amd/csrc/project.hip), strict IEEE (-ffp-contract=off):
 * Frame::isInFrustum / isInFrustumChecks (src/Frame.cc:548-637, :1252-1325), MapPoint::PredictScale (src/MapPoint.cc:570-593) and
 * the projection loops of ORBmatcher::SearchByProjection (src/ORBmatcher.cc:1999-2022, :2092-2095, :2215-2239), with the OpenCV
 * 3.4.1 choices of DESIGN.md section 2.  Test infrastructure: compiled into a temporary directory by tests/proj_ref/__init__.py, never
 * loaded by the product.  The KannalaBrandt8 projection is the oracle's (orc_camera_project, handed in through pr_set_project): its
 * atan2f / sinf / cosf restatements are checked against the device's on their whole domains already. */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct { int model; float fx, fy, cx, cy; float k[4]; float precision; } pr_camera;      /* = eorb_camera */
typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } pr_keypoint;    /* = eorb_keypoint */

typedef struct pr_view {                                                                          /* = eorb_view */
    float R[9], t[3], Ow[3];
    pr_camera cam;
    float minX, maxX, minY, maxY, mbf;
    int nlevels;    float log_scale;    const float* scale_factors;
    int ak_nlevels; float ak_log_scale; const float* ak_scale_factors;
} pr_view;

typedef struct pr_frustum_out {                                                                   /* = eorb_frustum_out + search */
    uint8_t* in_view; float* proj_xy; float* proj_xr; int32_t* level; float* view_cos; float* depth; float* level_scale; uint8_t* reason;
    uint8_t* search;       /* in_view and not beyond thFarPoints (ORBmatcher.cc:57): what the matcher is given as in_view */
} pr_frustum_out;

typedef void (*pr_project_fn)(const pr_camera*, const float*, float*, float*);
static pr_project_fn g_project = 0;
void pr_set_project(pr_project_fn f) { g_project = f; }

/* ---- glibc e_logf.c (>= 2.27) --------------------------------------------------------------------------------------------- */
static const struct { double invc, logc; } LOGF_T[16] = {
    { 0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2 }, { 0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2 },
    { 0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2 },  { 0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3 },
    { 0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3 }, { 0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3 },
    { 0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4 }, { 0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4 },
    { 0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5 }, { 0x1p+0, 0x0p+0 },
    { 0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5 },  { 0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4 },
    { 0x1.b2036576afce6p-1, 0x1.526e57720db08p-3 },  { 0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3 },
    { 0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2 },  { 0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2 },
};
static const double LOGF_LN2 = 0x1.62e42fefa39efp-1;
static const double LOGF_A[3] = { -0x1.00ea348b88334p-2, 0x1.5575b0be00b6ap-2, -0x1.ffffef20a4123p-2 };

static float bits_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t f_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

float pr_logf(float x)
{
    uint32_t ix = f_bits(x);
    if (ix == 0x3f800000u) return 0;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        if (ix * 2 == 0) return bits_f(0xff800000u);
        if (ix == 0x7f800000u) return x;
        if ((ix & 0x80000000u) || ix * 2 >= 0xff000000u) return bits_f(0x7fc00000u);
        ix = f_bits(x * 0x1p23f);
        ix -= 23u << 23;
    }
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (tmp >> 19) % 16;
    const int k = (int32_t)tmp >> 23;
    const uint32_t iz = ix - (tmp & (0x1ffu << 23));
    const double z = (double)bits_f(iz);
    const double r = z * LOGF_T[i].invc - 1;
    const double y0 = LOGF_T[i].logc + (double)k * LOGF_LN2;
    const double r2 = r * r;
    double y = LOGF_A[1] * r + LOGF_A[2];
    y = LOGF_A[0] * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}

void pr_logf_n(const float* x, long n, float* out) { for (long i = 0; i < n; i++) out[i] = pr_logf(x[i]); }

/* number of bit patterns in [lo, hi] on which pr_logf and the host logf differ; *first = the first of them */
uint64_t pr_logf_mismatches(uint32_t lo, uint32_t hi, uint32_t* first)
{
    uint64_t bad = 0;
    for (uint64_t u = lo; u <= hi; u++) {
        const volatile float x = bits_f((uint32_t)u);
        if (f_bits(pr_logf(x)) != f_bits(logf(x))) { if (!bad && first) *first = (uint32_t)u; bad++; }
    }
    return bad;
}

/* the hash of eorb_selfcheck_math (which = 6) */
uint64_t pr_math_hash(int which, uint32_t lo_bits, uint32_t hi_bits)
{
    uint64_t h = 0;
    if (which != 6) return 0;
    for (uint64_t u = lo_bits; u <= hi_bits; u++) {
        const uint32_t ub = (uint32_t)u;
        h += (((uint64_t)ub * 0x9E3779B97F4A7C15ull) ^ (uint64_t)f_bits(pr_logf(bits_f(ub)))) * 0xC2B2AE3D27D4EB4Full;
    }
    return h;
}

/* ---- OpenCV 3.4.1 scalar paths (as eorb_slam_amd/csrc/kb8_dev.h) ------------------------------------------------------------- */
/* gemm, len 3, d_size.width == 1: products summed in float, then (float)(t*alpha + c*beta) in double */
static void gemm3x1(const float* R, const float* x, const float* c, float* out)
{
    for (int i = 0; i < 3; i++) {
        const float t = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
        out[i] = (float)((double)t * 1.0 + (double)c[i] * 1.0);
    }
}
static double dot3(const float* a, const float* b)
{
    double s = 0;
    for (int i = 0; i < 3; i++) s += (double)a[i] * b[i];
    return 0.0 + s;
}
static double norm3(const float* a)
{
    double s = 0;
    for (int i = 0; i < 3; i++) { const double v = a[i]; s += v * v; }
    return sqrt(0 + s);
}
static void project(const pr_camera* c, const float* p, float* u, float* v)
{
    if (c->model == 0) { *u = c->fx * p[0] / p[2] + c->cx; *v = c->fy * p[1] / p[2] + c->cy; return; }
    g_project(c, p, u, v);
}
static int finite2(float u, float v) { return isfinite(u) && isfinite(v); }

/* MapPoint::PredictScale; a ceil() no int holds converts as cvttss2si does (INT_MIN -> 0 after the clamp) */
int pr_predict_scale(float max_dist, float dist, int nlevels, float log_scale)
{
    const float ratio = max_dist / dist;
    const float cf = ceilf(pr_logf(ratio) / log_scale);
    int n = (cf >= -2147483648.0f && cf < 2147483648.0f) ? (int)cf : INT_MIN;
    if (n < 0) n = 0;
    else if (n >= nlevels) n = nlevels - 1;
    return n;
}

static void tables(const pr_view* V, int is_orb, int* nlevels, float* log_scale, const float** sf)
{
    if (!is_orb && V->ak_nlevels > 0) { *nlevels = V->ak_nlevels; *log_scale = V->ak_log_scale; *sf = V->ak_scale_factors; }
    else { *nlevels = V->nlevels; *log_scale = V->log_scale; *sf = V->scale_factors; }
}

typedef struct { int in_view, reason, level; float x, y, xr, cos, depth, lscale; } rec_t;
static const rec_t REC0 = {0, 0, -1, -1.f, -1.f, 0.f, 0.f, 0.f, 0.f};

/* mode A, one view */
static rec_t frustum_view(const pr_view* V, const float* P, const float* Pn, float minD, float maxD, int is_orb, float lim)
{
    rec_t o = REC0;
    float Pc[3], u, v;
    gemm3x1(V->R, P, V->t, Pc);
    o.depth = (float)norm3(Pc);
    const float PcZ = Pc[2];
    if (PcZ < 0.0f) { o.reason = 2; return o; }
    project(&V->cam, Pc, &u, &v);
    if (!finite2(u, v)) { o.reason = 7; return o; }
    if (u < V->minX || u > V->maxX) { o.reason = 3; return o; }
    if (v < V->minY || v > V->maxY) { o.reason = 4; return o; }
    o.x = u; o.y = v;
    const float PO[3] = {P[0] - V->Ow[0], P[1] - V->Ow[1], P[2] - V->Ow[2]};
    const float dist = (float)norm3(PO);
    if (dist < 0.8f * minD || dist > 1.2f * maxD) { o.reason = 5; return o; }
    const float viewCos = (float)(dot3(PO, Pn) / (double)dist);
    o.cos = viewCos;
    if (viewCos < lim) { o.reason = 6; return o; }
    int nl; float lsf; const float* sf;
    tables(V, is_orb, &nl, &lsf, &sf);
    o.level = pr_predict_scale(maxD, dist, nl, lsf);
    o.lscale = sf[o.level];
    o.xr = u - V->mbf * (1.0f / PcZ);
    o.in_view = 1;
    return o;
}

static void store(const pr_frustum_out* O, long m, const rec_t* r, int search)
{
    if (O->in_view) O->in_view[m] = (uint8_t)r->in_view;
    if (O->proj_xy) { O->proj_xy[2 * m] = r->x; O->proj_xy[2 * m + 1] = r->y; }
    if (O->proj_xr) O->proj_xr[m] = r->xr;
    if (O->level) O->level[m] = r->level;
    if (O->view_cos) O->view_cos[m] = r->cos;
    if (O->depth) O->depth[m] = r->depth;
    if (O->level_scale) O->level_scale[m] = r->lscale;
    if (O->reason) O->reason[m] = (uint8_t)r->reason;
    if (O->search) O->search[m] = (uint8_t)search;
}

int pr_frustum(const pr_view* views, int nviews, long M, const float* pos, const float* normal, const float* min_dist,
               const float* max_dist, const uint8_t* skip, const uint8_t* is_orb, float cos_limit, int far, float th_far,
               const pr_frustum_out* out)
{
    int n_in_view = 0;
    for (long m = 0; m < M; m++) {
        rec_t r[2];
        if (skip && skip[m]) { r[0] = REC0; r[0].reason = 1; r[1] = r[0]; }
        else {
            const int io = is_orb ? is_orb[m] != 0 : 1;
            r[0] = frustum_view(views, pos + 3 * m, normal + 3 * m, min_dist[m], max_dist[m], io, cos_limit);
            r[1] = nviews > 1 ? frustum_view(views + 1, pos + 3 * m, normal + 3 * m, min_dist[m], max_dist[m], io, cos_limit) : r[0];
        }
        const float d = (nviews > 1 && !r[0].in_view) ? r[1].depth : r[0].depth;
        const int gate = far && d > th_far;
        store(out, m, &r[0], r[0].in_view && !gate);
        if (nviews > 1) store(out + 1, m, &r[1], r[1].in_view && !gate);
        n_in_view += r[0].in_view || (nviews > 1 && r[1].in_view);
    }
    return n_in_view;
}

/* mode B */
void pr_last(const pr_view* V, const pr_camera* cam_r, const float* Trl, long n, const float* pos, const uint8_t* skip,
             const pr_keypoint* kps, const uint8_t* is_orb, uint8_t* valid, float* uv, float* proj_ur, float* level_scale, float* uv_r)
{
    for (long i = 0; i < n; i++) {
        int nl; float lsf; const float* sf;
        tables(V, is_orb ? is_orb[i] != 0 : 1, &nl, &lsf, &sf);
        const float ls = sf[kps[i].octave];
        int ok = 0;
        float u = -1.f, v = -1.f, ur = 0.f, u_r = -1.f, v_r = -1.f;
        if (!(skip && skip[i])) {
            float x3Dc[3], pu, pv;
            gemm3x1(V->R, pos + 3 * i, V->t, x3Dc);
            const float invzc = (float)(1.0 / (double)x3Dc[2]);
            if (!(invzc < 0)) {
                project(&V->cam, x3Dc, &pu, &pv);
                if (finite2(pu, pv) && !(pu < V->minX || pu > V->maxX) && !(pv < V->minY || pv > V->maxY)) {
                    ok = 1; u = pu; v = pv;
                    ur = pu - V->mbf * invzc;
                    if (Trl) {
                        float x3Dr[3];
                        gemm3x1(Trl, x3Dc, Trl + 9, x3Dr);
                        project(cam_r, x3Dr, &u_r, &v_r);
                    }
                }
            }
        }
        if (valid) valid[i] = (uint8_t)ok;
        if (uv) { uv[2 * i] = u; uv[2 * i + 1] = v; }
        if (proj_ur) proj_ur[i] = ur;
        if (level_scale) level_scale[i] = ls;
        if (uv_r) { uv_r[2 * i] = u_r; uv_r[2 * i + 1] = v_r; }
    }
}

/* mode C */
void pr_kf(const pr_view* V, long n, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* skip,
           const uint8_t* is_orb, uint8_t* valid, float* uv, int32_t* level, float* level_scale, float* dist3d)
{
    for (long i = 0; i < n; i++) {
        int ok = 0, lv = -1;
        float u = -1.f, v = -1.f, ls = 0.f, d3 = 0.f;
        if (!(skip && skip[i])) {
            const float* P = pos + 3 * i;
            float x3Dc[3], pu, pv;
            gemm3x1(V->R, P, V->t, x3Dc);
            project(&V->cam, x3Dc, &pu, &pv);
            if (finite2(pu, pv) && !(pu < V->minX || pu > V->maxX) && !(pv < V->minY || pv > V->maxY)) {
                u = pu; v = pv;
                const float PO[3] = {P[0] - V->Ow[0], P[1] - V->Ow[1], P[2] - V->Ow[2]};
                d3 = (float)norm3(PO);
                if (!(d3 < 0.8f * min_dist[i] || d3 > 1.2f * max_dist[i])) {
                    int nl; float lsf; const float* sf;
                    tables(V, is_orb ? is_orb[i] != 0 : 1, &nl, &lsf, &sf);
                    lv = pr_predict_scale(max_dist[i], d3, nl, lsf);
                    ls = sf[lv];
                    ok = 1;
                }
            }
        }
        if (valid) valid[i] = (uint8_t)ok;
        if (uv) { uv[2 * i] = u; uv[2 * i + 1] = v; }
        if (level) level[i] = lv;
        if (level_scale) level_scale[i] = ls;
        if (dist3d) dist3d[i] = d3;
    }
}
