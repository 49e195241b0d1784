// Boundary terms on the device: the matrix of a boundary integral over one side of a patch is added to the
// volume values the patch -- or the sums of a multipatch -- hold in device memory.
//
//   k_face_add   one group of lanes per row of the face matrix (the group width chosen from the longest face row by the thresholds
//                of k_spmv's): the lanes read the row's values contiguously and do  vol[pos] += r  as a plain read-add-write.
//
// Position arithmetic.  The values of a patch are stored row after row, row I = (i0, i1, i2) holding the columns
// [jlo_0, jhi_0) x [jlo_1, jhi_1) x [jlo_2, jhi_2) lexicographically from igx_rowptr3 on (a 2D patch is a 3D one with a one-dof
// outer axis).  A side fixes i_a = j_a = f on the normal axis a; the face space is the tensor product of the other two axes
// (u, v), in their order, and its own values have the same layout one dimension down.  Face entry (ju, jv) of face row (u, v),
// counted from the row's first column, therefore sits in the volume row at
//       normal axis 0:  (jn cu + ju) cv + jv        a contiguous segment of cu cv values
//       normal axis 1:  (ju cn + jn) cv + jv        runs of cv values
//       normal axis 2:  (ju cv + jv) cn + jn        single values at stride cn
// with jn = f - jlo_a(f) and c. the column counts of the row: one offset  base + ju su + jv sv  whose three integers are worked
// out per row.  One kernel serves the three orientations -- they differ in those integers only.
// Within one face no two entries share a position, and calls run in stream order: no atomics, and where two faces meet the sum
// is ((a + r_1) + r_2) in the order of the calls.  On a multipatch the local position k is mapped through the patch's row plan
// (RowInfo): k + delta for rows stored directly, the position array otherwise; atomicAdd only where a map is not injective.
#include "igx_internal.h"

#include <algorithm>
#include <climits>

using namespace igx;

namespace {

constexpr int FBLOCK = 256;

struct FaceGeom {
    int Nu, Nv, Nn;                                  // dofs of the face axes (Nu = 1: a 1D face) and of the normal axis
    const int *jlo_u, *jhi_u, *rp_u;                 // per-axis tables of the face axes (device; u: null for a 1D face)
    const int *jlo_v, *jhi_v, *rp_v;
    long long Sv;                                    // 1D index pairs of axis v: the face's row pointer is rp_u Sv + cu rp_v
    int normal;                                      // place of the normal axis among the three of the volume layout
    int fn, jn, cn, rpn;                             // normal axis at the side: dof, its place in its row's columns, their number, rp
    long long S1, S2;                                // 1D index pairs of the volume's mid and last axis
    long long nrows;                                 // face rows = Nu Nv
};

template <bool MP>
__global__ void __launch_bounds__(FBLOCK) k_face_add(const FaceGeom g, int gw, const double *__restrict__ fvals, double *vals,
                                                    const RowInfo *__restrict__ info, const int32_t *__restrict__ cpos, int atomic)
{
    const int lane = threadIdx.x % gw;
    const long long It = ((long long)blockIdx.x * FBLOCK + threadIdx.x) / gw;
    if (It >= g.nrows) return;
    const int u = (int)(It / g.Nv), v = (int)(It % g.Nv);
    const int lu = g.jlo_u ? g.jlo_u[u] : 0, cu = g.jlo_u ? g.jhi_u[u] - lu : 1, ru = g.jlo_u ? g.rp_u[u] : 0;
    const int lv = g.jlo_v[v], cv = g.jhi_v[v] - lv, rv = g.rp_v[v];
    (void)lv;
    const double *src = fvals + ((long long)ru * g.Sv + (long long)cu * rv);
    // the volume row (i0, i1, i2): the normal axis takes its place among the face axes (uniform selects; the three orientations
    // share every instruction after them)
    const int n0 = g.normal == 0, n1 = g.normal == 1, n2 = g.normal == 2;
    const int i0 = n0 ? g.fn : u, r0 = n0 ? g.rpn : ru, c0 = n0 ? g.cn : cu;
    const int i1 = n0 ? u : n1 ? g.fn : v, r1 = n0 ? ru : n1 ? g.rpn : rv, c1 = n0 ? cu : n1 ? g.cn : cv;
    const int i2 = n2 ? g.fn : v, r2 = n2 ? g.rpn : rv, c2 = n2 ? g.cn : cv;
    const int N1 = n0 ? g.Nu : n1 ? g.Nn : g.Nv, N2 = n2 ? g.Nn : g.Nv;
    const long long row = (long long)r0 * g.S1 * g.S2 + (long long)c0 * ((long long)r1 * g.S2 + (long long)c1 * r2);
    const long long I = ((long long)i0 * N1 + i1) * N2 + i2;
    // column (j0, j1, j2) of the row sits at (j0 c1 + j1) c2 + j2: strides c1 c2, c2, 1 for the three places
    const int st0 = c1 * c2, st1 = c2;
    const int su = n0 ? st1 : st0, sv = n2 ? st1 : 1, base = g.jn * (n0 ? st0 : n1 ? st1 : 1);
    const int len = cu * cv;
    if (!MP) {
        double *dst = vals + row + base;
        for (int e = lane; e < len; e += gw) {
            const int ju = e / cv, jv = e - ju * cv;
            dst[(long long)ju * su + jv * sv] += src[e];
        }
        return;
    }
    const RowInfo ri = info[I];
    for (int e = lane; e < len; e += gw) {
        const int ju = e / cv, jv = e - ju * cv;
        const long long k = row + base + (long long)ju * su + jv * sv;       // position among the patch's own values
        const long long pos = ri.mode == MODE_DIRECT ? k + ri.base : (long long)cpos[ri.base + (k - ri.kstart)];
        if (atomic) atomicAdd(&vals[pos], src[e]);
        else vals[pos] += src[e];
    }
}

int face_gw(long long maxlen)                        // (the thresholds of the SpMV's group width, solve.hip)
{
    return maxlen >= 192 ? 64 : maxlen >= 96 ? 32 : maxlen >= 48 ? 16 : maxlen >= 24 ? 8 : 4;
}

// one axis of a value layout: host tables and their device copies
struct AxView {
    int N, p;
    const std::vector<int> *jlo, *jhi, *rp;
    const int *d_jlo, *d_jhi, *d_rp;
};

AxView view_of(const igx_patch *pt, int k)
{
    const Axis &A = pt->ax[k];
    return AxView{A.N, A.p, &A.jlo, &A.jhi, &A.rp, A.dev.jlo, A.dev.jhi, A.dev.rp};
}

// The launch geometry of side (axis, side) of a volume of `dim` axes `vol`; *nvals: values of the face matrix; *gw: group width.
int face_geom(const char *what, int dim, const AxView *vol, int axis, int side, FaceGeom &g, long long *nvals, int *gw)
{
    if (axis < 0 || axis >= dim || (side != 0 && side != 1)) {
        set_error("%s: side (%d, %d) of a %dD patch: axis 0 .. %d, side 0 or 1", what, axis, side, dim, dim - 1);
        return IGX_ERR_ARG;
    }
    const int off = 3 - dim;
    const AxView &n = vol[axis];
    g.normal = axis + off;
    g.Nn = n.N;
    g.fn = side ? n.N - 1 : 0;
    g.jn = g.fn - (*n.jlo)[g.fn];
    g.cn = (*n.jhi)[g.fn] - (*n.jlo)[g.fn];
    g.rpn = (*n.rp)[g.fn];
    const AxView *t[2] = {nullptr, nullptr};         // the face axes u, v (u absent for a 1D face)
    int nt = 0;
    for (int k = 0; k < dim; ++k)
        if (k != axis) t[nt++] = &vol[k];
    const AxView *U = nt == 2 ? t[0] : nullptr, *V = nt == 2 ? t[1] : t[0];
    g.Nu = U ? U->N : 1;
    g.Nv = V->N;
    g.jlo_u = U ? U->d_jlo : nullptr; g.jhi_u = U ? U->d_jhi : nullptr; g.rp_u = U ? U->d_rp : nullptr;
    g.jlo_v = V->d_jlo; g.jhi_v = V->d_jhi; g.rp_v = V->d_rp;
    g.Sv = (*V->rp)[V->N];
    // pairs of the volume's mid and last axis (3D layout: the axes of a 2D patch are its mid and last)
    g.S1 = (*vol[dim - 2].rp)[vol[dim - 2].N];
    g.S2 = (*vol[dim - 1].rp)[vol[dim - 1].N];
    g.nrows = (long long)g.Nu * g.Nv;
    *nvals = (U ? (long long)(*U->rp)[U->N] : 1LL) * g.Sv;
    long long maxlen = 1;
    for (int a = 0; a < nt; ++a) {
        int mc = 0;
        for (int i = 0; i < t[a]->N; ++i) mc = std::max(mc, (*t[a]->jhi)[i] - (*t[a]->jlo)[i]);
        maxlen *= mc;
    }
    *gw = face_gw(maxlen);
    if (g.nrows * *gw / FBLOCK + 1 >= INT_MAX) { set_error("%s: face of %lld rows too large", what, g.nrows); return IGX_ERR_UNSUPPORTED; }
    return IGX_OK;
}

// the face patch against the volume's other axes: dimension, whole patch, values, degrees, dof counts, column ranges
int check_face(const char *what, const igx_ctx *ctx, int dim, const AxView *vol, int axis, const igx_patch *face)
{
    if (face->ctx != ctx) { set_error("%s: the face patch lives on another context", what); return IGX_ERR_ARG; }
    if (face->boxed || face->row_lo != 0 || face->row_hi != face->nrows_total) {
        set_error("%s: whole patches only (the face patch is a row slab or span box)", what);
        return IGX_ERR_UNSUPPORTED;
    }
    if (face->dim != dim - 1) {
        set_error("%s: a %dD patch takes a %dD face patch, not a %dD one (the 1D faces of 2D patches: the _host variant)", what, dim, dim - 1, face->dim);
        return IGX_ERR_ARG;
    }
    if (!face->d_data || face->values_kind < 0) { set_error("%s: the face patch holds no assembled values", what); return IGX_ERR_ARG; }
    for (int k = 0, a = 0; k < dim; ++k) {
        if (k == axis) continue;
        const Axis &F = face->ax[a];
        const AxView &W = vol[k];
        if (F.p != W.p || F.N != W.N || F.jlo != *W.jlo || F.jhi != *W.jhi) {
            set_error("%s: axis %d of the face patch (degree %d, %d dofs) is not axis %d of the patch (degree %d, %d dofs): degrees, "
                      "dof counts and column ranges must agree", what, a, F.p, F.N, k, W.p, W.N);
            return IGX_ERR_ARG;
        }
        ++a;
    }
    return IGX_OK;
}

// host values through a staging buffer of their own (face matrices are small next to the volume's values)
int stage_values(const char *what, hipStream_t st, const double *vals, long long n, double **d_out)
{
    *d_out = nullptr;
    if (hipMalloc((void **)d_out, std::max<size_t>(1, (size_t)n) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: hipMalloc of %.3f GB for the face values failed", what, n * 8.0 / 1e9);
        return IGX_ERR_NOMEM;
    }
    hipError_t e = hipMemcpyAsync(*d_out, vals, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(*d_out); *d_out = nullptr; set_error("%s: %s", what, hipGetErrorString(e)); return IGX_ERR_HIP; }
    return IGX_OK;
}

unsigned face_grid(const FaceGeom &g, int gw) { return (unsigned)((g.nrows * gw + FBLOCK - 1) / FBLOCK); }

// ---- one patch
int patch_prepare(const char *what, igx_patch *pt, int axis, int side, AxView vol[3], FaceGeom &g, long long *nvals, int *gw)
{
    if (pt->boxed || pt->row_lo != 0 || pt->row_hi != pt->nrows_total) {
        set_error("%s: whole patches only (no row slab, no span box)", what);
        return IGX_ERR_UNSUPPORTED;
    }
    if (pt->values_kind < 0 || !pt->d_data) { set_error("%s: the patch holds no assembled values (igx_assemble first)", what); return IGX_ERR_ARG; }
    for (int k = 0; k < pt->dim; ++k) vol[k] = view_of(pt, k);
    return face_geom(what, pt->dim, vol, axis, side, g, nvals, gw);
}

int patch_add(igx_patch *pt, const FaceGeom &g, int gw, const double *d_face)
{
    hipStream_t st = pt->ctx->stream;
    hipEvent_t *ev = pt->ctx->ev;
    IGX_HIP(hipEventRecord(ev[0], st));
    if (g.nrows) k_face_add<false><<<face_grid(g, gw), FBLOCK, 0, st>>>(g, gw, d_face, pt->d_data, nullptr, nullptr, 0);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipEventRecord(ev[1], st));
    IGX_HIP(hipStreamSynchronize(st));               // (the face patch or the staging buffer may be freed after the call)
    pt->timing = igx_timing{};                       // igx_last_timing: the device time of the add
    (void)hipEventElapsedTime(&pt->timing.total_ms, ev[0], ev[1]);
    pt->timing.algo_used = 7;
    pt->timing.n_launches = 1;
    return IGX_OK;
}

// ---- multipatch
int mp_prepare(const char *what, igx_multipatch *mp, int p, int axis, int side, AxView vol[3], FaceGeom &g, long long *nvals, int *gw)
{
    if (p < 0 || p >= mp->np) { set_error("%s: patch %d out of range", what, p); return IGX_ERR_ARG; }
    auto &P = mp->pp[p];
    if (axis < 0 || axis >= P.dim || (side != 0 && side != 1)) {
        set_error("%s: side (%d, %d) of a %dD patch: axis 0 .. %d, side 0 or 1", what, axis, side, P.dim, P.dim - 1);
        return IGX_ERR_ARG;
    }
    if (P.scattered != mp->generation) {
        set_error("%s: patch %d has not been scattered into the current sums (its scatter would overwrite the add)", what, p);
        return IGX_ERR_ARG;
    }
    IGX_HIP(hipSetDevice(mp->ctx->device));
    if (!P.d_tab) {                                  // the patch's per-axis tables, uploaded when a face is first added
        std::vector<int> tab;
        for (int k = 0; k < P.dim; ++k) {
            P.tab_pos[k][0] = tab.size(); tab.insert(tab.end(), P.jlo[k].begin(), P.jlo[k].end());
            P.tab_pos[k][1] = tab.size(); tab.insert(tab.end(), P.jhi[k].begin(), P.jhi[k].end());
            P.tab_pos[k][2] = tab.size(); tab.insert(tab.end(), P.rp[k].begin(), P.rp[k].end());
        }
        if (hipMalloc((void **)&P.d_tab, tab.size() * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError(); P.d_tab = nullptr;
            set_error("%s: out of device memory", what);
            return IGX_ERR_NOMEM;
        }
        hipError_t e = hipMemcpyAsync(P.d_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, mp->ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(mp->ctx->stream);
        if (e != hipSuccess) { (void)hipFree(P.d_tab); P.d_tab = nullptr; set_error("%s: %s", what, hipGetErrorString(e)); return IGX_ERR_HIP; }
    }
    for (int k = 0; k < P.dim; ++k)
        vol[k] = AxView{P.N[k], P.p[k], &P.jlo[k], &P.jhi[k], &P.rp[k], P.d_tab + P.tab_pos[k][0], P.d_tab + P.tab_pos[k][1], P.d_tab + P.tab_pos[k][2]};
    return face_geom(what, P.dim, vol, axis, side, g, nvals, gw);
}

int mp_add(igx_multipatch *mp, int p, const FaceGeom &g, int gw, const double *d_face)
{
    hipStream_t st = mp->ctx->stream;
    const auto &P = mp->pp[p];
    if (g.nrows) k_face_add<true><<<face_grid(g, gw), FBLOCK, 0, st>>>(g, gw, d_face, mp->d_vals, P.d_info, P.d_cpos, mp->injective ? 0 : 1);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

} // namespace

extern "C" {

int igx_patch_add_face(igx_patch *patch, int axis, int side, const igx_patch *face)
{
    const char *what = "igx_patch_add_face";
    if (!patch || !face) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    AxView vol[3];
    FaceGeom g{};
    long long nvals = 0;
    int gw = 4;
    if (int rc = patch_prepare(what, patch, axis, side, vol, g, &nvals, &gw)) return rc;
    if (int rc = check_face(what, patch->ctx, patch->dim, vol, axis, face)) return rc;
    IGX_HIP(hipSetDevice(patch->ctx->device));
    return patch_add(patch, g, gw, face->d_data);
}

int igx_patch_add_face_host(igx_patch *patch, int axis, int side, const double *vals, int64_t nvals)
{
    const char *what = "igx_patch_add_face_host";
    if (!patch || !vals) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    AxView vol[3];
    FaceGeom g{};
    long long want = 0;
    int gw = 4;
    if (int rc = patch_prepare(what, patch, axis, side, vol, g, &want, &gw)) return rc;
    if (nvals != want) { set_error("%s: %lld values given, the face matrix has %lld", what, (long long)nvals, want); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(patch->ctx->device));
    double *d_face = nullptr;
    if (int rc = stage_values(what, patch->ctx->stream, vals, want, &d_face)) return rc;
    const int rc = patch_add(patch, g, gw, d_face);
    (void)hipFree(d_face);
    return rc;
}

int igx_multipatch_add_face(igx_multipatch *mp, int p, int axis, int side, const igx_patch *face)
{
    const char *what = "igx_multipatch_add_face";
    if (!mp || !face) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    AxView vol[3];
    FaceGeom g{};
    long long nvals = 0;
    int gw = 4;
    if (int rc = mp_prepare(what, mp, p, axis, side, vol, g, &nvals, &gw)) return rc;
    if (int rc = check_face(what, mp->ctx, mp->pp[p].dim, vol, axis, face)) return rc;
    return mp_add(mp, p, g, gw, face->d_data);
}

int igx_multipatch_add_face_host(igx_multipatch *mp, int p, int axis, int side, const double *vals, int64_t nvals)
{
    const char *what = "igx_multipatch_add_face_host";
    if (!mp || !vals) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    AxView vol[3];
    FaceGeom g{};
    long long want = 0;
    int gw = 4;
    if (int rc = mp_prepare(what, mp, p, axis, side, vol, g, &want, &gw)) return rc;
    if (nvals != want) { set_error("%s: %lld values given, the face matrix has %lld", what, (long long)nvals, want); return IGX_ERR_ARG; }
    double *d_face = nullptr;
    if (int rc = stage_values(what, mp->ctx->stream, vals, want, &d_face)) return rc;
    const int rc = mp_add(mp, p, g, gw, d_face);
    (void)hipFree(d_face);
    return rc;
}

} // extern "C"
