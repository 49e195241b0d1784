// igx_pair: bilinear forms over TWO tensor-product spline spaces on one mesh (Taylor-Hood pairs, Q1-P0, ...).
//
// A pair is a full patch -- the TRIAL space (columns), which owns the geometry, the Gauss grid and the form fields -- plus a
// TEST space (rows) given by per-axis degree and open knot vector with exactly the patch's breakpoints.  The reference's
// generated assemblers always take rows from space 1 and columns from space 0 and integrate on the mesh of space 0
// (pyiga/genericasm.pxi, "we assume all kvs result in the same mesh"); unequal meshes are refused here.
//
// The matrix is rectangular, prod(N_test) x prod(N_trial), canonical CSR with exactly the product pattern: row (i0, i1[, i2])
// holds the columns [jlo_0, jhi_0) x [jlo_1, jhi_1) [x ..] in lexicographic order, [jlo_k, jhi_k) = the trial functions of axis
// k whose mesh support meets that of test function i_k.  With the per-axis prefix sums rp_k of (jhi_k - jlo_k) the row pointer
// is igx_rowptr3 as for a square patch (DESIGN.md "CSR pattern without index arrays").
//
// Kernels: one thread = one entry, summed over the intersection of the two supports with the loops nested axis 0 outermost and
// a single accumulator -- the reference's order, the expressions of entry_value (kern_entries.hip) with the u factors from the
// trial tables and the v factors from the test tables.  No mirror, no triangle: every entry of every row is computed once.
#include "pair_internal.h"
#include <algorithm>
#include <cstring>
#include <new>

namespace igx {

// grid.x * block.x of one launch stays below 2^32 (the limit of the HIP runtimes this library supports)
constexpr long long PAIR_MAX_THREADS = 0xFFFFFFFFll;

template <int DIM>
__device__ inline bool pair_unravel(int N0, int N1, int N2, size_t I, int out[3])
{
    if (DIM == 3) { out[2] = (int)(I % (size_t)N2); I /= (size_t)N2; } else out[2] = 0;
    out[1] = (int)(I % (size_t)N1);
    const size_t r = I / (size_t)N1;
    out[0] = (int)r;
    return r < (size_t)N0;
}

// entry (test i, trial j); the patch of a pair is whole (no slab, no box): every Gauss point is resident
template <int DIM, int KIND>
__device__ inline double pair_entry_value(const PatchDev &pd, const PairDev &pr, const double *fields, const int i[3], const int j[3])
{
    int glo[3], ghi[3];
    for (int k = 0; k < DIM; ++k) {
        const AxisDev &A = pd.ax[k];
        const PairAxisDev &T = pr.t[k];
        const int lo = max(T.mslo[i[k]], A.mslo[j[k]]);
        const int hi = min(T.mshi[i[k]], A.mshi[j[k]]);
        if (lo >= hi) return 0.0;                     // no intersection of supports
        glo[k] = lo * A.q; ghi[k] = hi * A.q;
    }
    const AxisDev &A0 = pd.ax[0], &A1 = pd.ax[1], &A2 = pd.ax[2];
    const PairAxisDev &T0 = pr.t[0], &T1 = pr.t[1], &T2 = pr.t[2];
    const long long stride = pd.npts_loc;
    double r = 0.0;
    for (int g0 = glo[0]; g0 < ghi[0]; ++g0) {
        const int s0 = g0 / A0.q;
        const double *u0 = A0.V + ((size_t)g0 * A0.P + (j[0] - A0.fa[s0])) * 2;
        const double *v0 = T0.V + ((size_t)g0 * T0.P + (i[0] - T0.fa[s0])) * 2;
        for (int g1 = glo[1]; g1 < ghi[1]; ++g1) {
            const int s1 = g1 / A1.q;
            const double *u1 = A1.V + ((size_t)g1 * A1.P + (j[1] - A1.fa[s1])) * 2;
            const double *v1 = T1.V + ((size_t)g1 * T1.P + (i[1] - T1.fa[s1])) * 2;
            if (DIM == 2) {
                const long long pt = (long long)g0 * pd.L1 + g1;
                if (KIND == IGX_MASS) {
                    r += (((u0[0] * u1[0]) * (v0[0] * v1[0])) * fields[pt]);
                } else {
                    // jets in parametric (x, y) order: 0 = value, 1 = d/dx (last grid axis), 2 = d/dy
                    const double Du[3] = {u0[0] * u1[0], u0[0] * u1[1], u0[1] * u1[0]};
                    const double Dv[3] = {v0[0] * v1[0], v0[0] * v1[1], v0[1] * v1[0]};
                    double e = 0.0;
                    for (int t = 0; t < pd.form_n; ++t) {
                        const int ab = pd.form_ab[t];
                        double dv = Dv[0], du = Du[0];
#pragma unroll
                        for (int c = 1; c < 3; ++c) { if ((ab >> 2) == c) dv = Dv[c]; if ((ab & 3) == c) du = Du[c]; }
                        e += (fields[t * stride + pt] * du) * dv;
                    }
                    r += e;
                }
            } else {
                for (int g2 = glo[2]; g2 < ghi[2]; ++g2) {
                    const int s2 = g2 / A2.q;
                    const double *u2 = A2.V + ((size_t)g2 * A2.P + (j[2] - A2.fa[s2])) * 2;
                    const double *v2 = T2.V + ((size_t)g2 * T2.P + (i[2] - T2.fa[s2])) * 2;
                    const long long pt = ((long long)g0 * pd.L1 + g1) * pd.L2 + g2;
                    if (KIND == IGX_MASS) {
                        r += (((u0[0] * u1[0] * u2[0]) * (v0[0] * v1[0] * v2[0])) * fields[pt]);
                    } else {
                        // jets in parametric (x, y, z) order: index 0 = value, 1 = d/dx (last grid axis), 2 = d/dy, 3 = d/dz
                        const double Du[4] = {u0[0] * u1[0] * u2[0], u0[0] * u1[0] * u2[1], u0[0] * u1[1] * u2[0], u0[1] * u1[0] * u2[0]};
                        const double Dv[4] = {v0[0] * v1[0] * v2[0], v0[0] * v1[0] * v2[1], v0[0] * v1[1] * v2[0], v0[1] * v1[0] * v2[0]};
                        double e = 0.0;
                        for (int t = 0; t < pd.form_n; ++t) {
                            const int ab = pd.form_ab[t];
                            double dv = Dv[0], du = Du[0];
#pragma unroll
                            for (int c = 1; c < 4; ++c) { if ((ab >> 2) == c) dv = Dv[c]; if ((ab & 3) == c) du = Du[c]; }
                            e += (fields[t * stride + pt] * du) * dv;
                        }
                        r += e;
                    }
                }
            }
        }
    }
    return r;
}

template <int DIM, int KIND>
__global__ void __launch_bounds__(128) k_pair_entries_list(PatchDev pd, PairDev pr, const double *fields, const size_t *ij, size_t M, double *out)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M) return;
    int i[3], j[3];
    const bool ok_i = pair_unravel<DIM>(pr.t[0].N, pr.t[1].N, pr.t[2].N, ij[2 * k], i);
    const bool ok_j = pair_unravel<DIM>(pd.ax[0].N, pd.ax[1].N, pd.ax[2].N, ij[2 * k + 1], j);
    out[k] = (ok_i && ok_j) ? pair_entry_value<DIM, KIND>(pd, pr, fields, i, j) : 0.0;
}

// start of row i in the CSR values and its per-axis column counts
template <int DIM>
__device__ inline long long pair_row_start(const PairDev &pr, const int i[3], int c[3])
{
    for (int k = 0; k < DIM; ++k) c[k] = pr.t[k].jhi[i[k]] - pr.t[k].jlo[i[k]];
    if (DIM == 2) return (long long)pr.t[0].rp[i[0]] * pr.t[1].S + (long long)c[0] * pr.t[1].rp[i[1]];
    return igx_rowptr3(pr.t[0].rp, pr.t[1].rp, pr.t[2].rp, pr.t[1].S, pr.t[2].S, c[0], c[1], i[0], i[1], i[2]);
}

// thread (row, offset < maxrow): rows unravelled by the test Ns, columns ravelled by the trial Ns
template <int DIM>
__global__ void __launch_bounds__(256) k_pair_pattern(PatchDev pd, PairDev pr, long long nrows, long long nnz, int maxrow, int32_t *indptr, int32_t *indices)
{
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = tid / maxrow;
    const int o = (int)(tid % maxrow);
    if (row > nrows) return;
    if (row == nrows) {                              // closing indptr entry
        if (o == 0) indptr[nrows] = (int32_t)nnz;
        return;
    }
    int i[3], c[3];
    pair_unravel<DIM>(pr.t[0].N, pr.t[1].N, pr.t[2].N, (size_t)row, i);
    const long long st = pair_row_start<DIM>(pr, i, c);
    const int len = c[0] * c[1] * (DIM == 3 ? c[2] : 1);
    if (o == 0) indptr[row] = (int32_t)st;
    if (o >= len) return;
    int j[3], rem = o;
    if (DIM == 3) { j[2] = pr.t[2].jlo[i[2]] + rem % c[2]; rem /= c[2]; }
    j[1] = pr.t[1].jlo[i[1]] + rem % c[1]; rem /= c[1];
    j[0] = pr.t[0].jlo[i[0]] + rem;
    long long J = (long long)j[0] * pd.ax[1].N + j[1];
    if (DIM == 3) J = J * pd.ax[2].N + j[2];
    indices[st + o] = (int32_t)J;
}

template <int DIM, int KIND>
__global__ void __launch_bounds__(128) k_pair_entries_csr(PatchDev pd, PairDev pr, const double *fields, long long nrows, int maxrow, double *data)
{
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = tid / maxrow;
    const int o = (int)(tid % maxrow);
    if (row >= nrows) return;
    int i[3], c[3], j[3];
    pair_unravel<DIM>(pr.t[0].N, pr.t[1].N, pr.t[2].N, (size_t)row, i);
    const long long st = pair_row_start<DIM>(pr, i, c);
    const int len = c[0] * c[1] * (DIM == 3 ? c[2] : 1);
    if (o >= len) return;
    int rem = o;
    if (DIM == 3) { j[2] = pr.t[2].jlo[i[2]] + rem % c[2]; rem /= c[2]; } else j[2] = 0;
    j[1] = pr.t[1].jlo[i[1]] + rem % c[1]; rem /= c[1];
    j[0] = pr.t[0].jlo[i[0]] + rem;
    data[st + o] = pair_entry_value<DIM, KIND>(pd, pr, fields, i, j);
}

} // namespace igx

using namespace igx;

// what the kernels assume of the patch at every call: checked again because the patch can be changed after igx_pair_create
static int pair_patch_ok(const igx_pair *pr, int kind, const char *who)
{
    const igx_patch *pt = pr->pt;
    if (kind != IGX_MASS && kind != IGX_FORM) { set_error("%s: kind must be IGX_MASS or IGX_FORM (got %d)", who, kind); return IGX_ERR_ARG; }
    if (!pt->basis_default) { set_error("%s: the patch's basis tables hold derivative orders other than (0, 1)", who); return IGX_ERR_UNSUPPORTED; }
    if (kind == IGX_FORM && pt->dev.form_par) { set_error("%s: a parametric jet form (igx_patch_set_pform) is not supported over two spaces", who); return IGX_ERR_UNSUPPORTED; }
    return IGX_OK;
}

static int pair_launch_fits(long long threads, const char *who)
{
    if (threads <= PAIR_MAX_THREADS) return IGX_OK;
    set_error("%s: %lld threads in one launch exceed the grid limit", who, threads);
    return IGX_ERR_UNSUPPORTED;
}

extern "C" {

void igx_pair_destroy(igx_pair *pr)
{
    if (!pr) return;
    (void)hipSetDevice(pr->ctx->device);
    (void)hipStreamSynchronize(pr->ctx->stream);
    for (int k = 0; k < 3; ++k) { (void)hipFree(pr->d_kv[k]); (void)hipFree(pr->d_V[k]); (void)hipFree(pr->d_ints[k]); }
    (void)hipFree(pr->d_data); (void)hipFree(pr->d_indptr); (void)hipFree(pr->d_indices); (void)hipFree(pr->d_ws_ij); (void)hipFree(pr->d_ws_out);
    delete pr;
}

static int pair_upload_axis(igx_pair *pr, int k, hipStream_t st)
{
    const Axis &T = pr->tax[k], &A = pr->pt->ax[k];
    IGX_HIP(hipMalloc((void **)&pr->d_kv[k], T.kv.size() * sizeof(double)));
    IGX_HIP(hipMemcpyAsync(pr->d_kv[k], T.kv.data(), T.kv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    std::vector<int> ints;
    auto app = [&](const int *v, size_t n) { size_t o = ints.size(); ints.insert(ints.end(), v, v + n); return o; };
    const size_t o_fa = app(T.fa.data(), T.n), o_lo = app(T.mslo.data(), T.N), o_hi = app(T.mshi.data(), T.N);
    const size_t o_jl = app(pr->jlo[k].data(), T.N), o_jh = app(pr->jhi[k].data(), T.N), o_rp = app(pr->rp[k].data(), T.N + 1);
    IGX_HIP(hipMalloc((void **)&pr->d_ints[k], ints.size() * sizeof(int)));
    IGX_HIP(hipMemcpyAsync(pr->d_ints[k], ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, st));
    // the test functions at the PATCH's Gauss nodes, by the kernel that fills the patch's own tables
    IGX_HIP(hipMalloc((void **)&pr->d_V[k], (size_t)A.G * T.P * 2 * sizeof(double)));
    if (int rc = launch_basis_tables(st, pr->d_kv[k], (int)T.kv.size(), T.p, A.d_nodes, (size_t)A.G, 1, nullptr, pr->d_V[k], nullptr, nullptr)) return rc;
    PairAxisDev &D = pr->dev.t[k];
    D.P = T.P; D.N = T.N; D.S = pr->rp[k][T.N];
    D.V = pr->d_V[k];
    D.fa = pr->d_ints[k] + o_fa; D.mslo = pr->d_ints[k] + o_lo; D.mshi = pr->d_ints[k] + o_hi;
    D.jlo = pr->d_ints[k] + o_jl; D.jhi = pr->d_ints[k] + o_jh; D.rp = pr->d_ints[k] + o_rp;
    IGX_HIP(hipStreamSynchronize(st));            // `ints` is a local buffer
    return IGX_OK;
}

igx_pair *igx_pair_create(igx_patch *pt, int dim, const int32_t *p, const int32_t *kv_len, const double *const *kv)
{
    if (!pt || !p || !kv_len || !kv) { set_error("igx_pair_create: null argument"); return nullptr; }
    if (dim != pt->dim) { set_error("igx_pair_create: the test space has dimension %d, the patch %d", dim, pt->dim); return nullptr; }
    if (pt->boxed) { set_error("igx_pair_create: the patch holds a span box"); return nullptr; }
    if (pt->r0_lo != 0 || pt->r0_hi != pt->ax[0].N) { set_error("igx_pair_create: the patch is a row slab [%d,%d) of %d dof planes", pt->r0_lo, pt->r0_hi, pt->ax[0].N); return nullptr; }
    if (pt->is_twin) { set_error("igx_pair_create: the patch is the axis-exchanged twin of another patch"); return nullptr; }
    if (!pt->basis_default) { set_error("igx_pair_create: the patch's basis tables hold derivative orders other than (0, 1)"); return nullptr; }
    igx_pair *pr = new (std::nothrow) igx_pair();
    if (!pr) { set_error("igx_pair_create: out of memory"); return nullptr; }
    pr->pt = pt;
    pr->ctx = pt->ctx;
    pr->dim = dim;
    const std::vector<double> unused(pt->nqp, 0.0);              // setup_axis also lays out a Gauss rule: the pair reads the patch's nodes instead
    for (int k = 0; k < dim; ++k) {
        Axis &T = pr->tax[k];
        const Axis &A = pt->ax[k];
        if (!kv[k]) { set_error("igx_pair_create: kv[%d] is null", k); delete pr; return nullptr; }
        if (setup_axis(T, kv[k], kv_len[k], p[k], pt->nqp, unused.data(), unused.data())) {      // (degree > IGX_MAX_DEGREE, not open, ..: its message)
            const std::string why = igx_last_error();
            set_error("igx_pair_create: test space, axis %d: %s", k, why.c_str());
            delete pr; return nullptr;
        }
        T.nodes = A.nodes; T.weights = A.weights;
        if (T.mesh != A.mesh) {
            set_error("igx_pair_create: axis %d: the breakpoints of the test space (%d spans) differ from the patch's (%d spans)", k, T.n, A.n);
            delete pr; return nullptr;
        }
        // trial columns of test row i: supports are monotone along the axis, so the overlapping trial functions are a range
        pr->jlo[k].resize(T.N); pr->jhi[k].resize(T.N); pr->rp[k].assign(T.N + 1, 0);
        for (int i = 0; i < T.N; ++i) {
            int lo = 0, hi = A.N;
            while (lo < A.N && A.mshi[lo] <= T.mslo[i]) ++lo;
            while (hi > lo && A.mslo[hi - 1] >= T.mshi[i]) --hi;
            pr->jlo[k][i] = lo; pr->jhi[k][i] = hi;
            pr->rp[k][i + 1] = pr->rp[k][i] + (hi - lo);
        }
    }
    pr->nrows = pr->ncols = pr->nnz = 1;
    long long maxrow = 1;
    for (int k = 0; k < dim; ++k) {
        pr->nrows *= pr->tax[k].N; pr->ncols *= pt->ax[k].N;
        int mk = 0;
        for (int i = 0; i < pr->tax[k].N; ++i) mk = std::max(mk, pr->jhi[k][i] - pr->jlo[k][i]);
        maxrow *= mk;
        // (S_k <= N_test * N_trial < 2^62 / ..: the product is formed in double first so that it cannot wrap)
        if ((double)pr->nnz * (double)pr->rp[k][pr->tax[k].N] > 9.0e18) { set_error("igx_pair_create: the pattern has more than 2^63 entries"); delete pr; return nullptr; }
        pr->nnz *= pr->rp[k][pr->tax[k].N];
    }
    pr->maxrow = (int)maxrow;                     // <= prod (2 p_trial + p_test + 1) <= 46^3
    if (hipSetDevice(pt->ctx->device) != hipSuccess) { set_error("igx_pair_create: hipSetDevice failed"); delete pr; return nullptr; }
    for (int k = 0; k < 3; ++k) { pr->dev.t[k].P = 1; pr->dev.t[k].N = 1; pr->dev.t[k].S = 1; }      // neutral third axis of a 2D pair
    for (int k = 0; k < dim; ++k)
        if (pair_upload_axis(pr, k, pt->ctx->stream)) { igx_pair_destroy(pr); return nullptr; }
    return pr;
}

int igx_pair_get_info(const igx_pair *pr, igx_pair_info *info)
{
    if (!pr || !info) { set_error("igx_pair_get_info: null argument"); return IGX_ERR_ARG; }
    memset(info, 0, sizeof(*info));
    info->dim = pr->dim;
    for (int k = 0; k < pr->dim; ++k) { info->ndofs_trial[k] = pr->pt->ax[k].N; info->ndofs_test[k] = pr->tax[k].N; }
    info->nrows = pr->nrows; info->ncols = pr->ncols; info->nnz = pr->nnz;
    return IGX_OK;
}

int igx_pair_pattern(igx_pair *pr, int32_t *indptr, int32_t *indices)
{
    if (!pr) { set_error("igx_pair_pattern: null pair"); return IGX_ERR_ARG; }
    if (pr->nnz > 0x7fffffffLL || pr->ncols > 0x7fffffffLL) {
        set_error("igx_pair_pattern: %lld nonzeros, %lld columns; int32 CSR indices need < 2^31", pr->nnz, pr->ncols);
        return IGX_ERR_UNSUPPORTED;
    }
    const long long total = (pr->nrows + 1) * pr->maxrow;
    if (int rc = pair_launch_fits(total + 255, "igx_pair_pattern")) return rc;
    igx_patch *pt = pr->pt;
    IGX_HIP(hipSetDevice(pt->ctx->device));
    hipStream_t st = pt->ctx->stream;
    if (!pr->have_pattern) {
        if (!pr->d_indptr) IGX_HIP(hipMalloc((void **)&pr->d_indptr, (size_t)(pr->nrows + 1) * sizeof(int32_t)));
        if (!pr->d_indices && hipMalloc((void **)&pr->d_indices, std::max<size_t>(1, (size_t)pr->nnz) * sizeof(int32_t)) != hipSuccess) {
            pr->d_indices = nullptr;
            set_error("hipMalloc of %.2f GB for CSR indices failed", pr->nnz * 4.0 / 1e9);
            return IGX_ERR_NOMEM;
        }
        dim3 grid((unsigned)((total + 255) / 256)), block(256);
        if (pr->dim == 2) k_pair_pattern<2><<<grid, block, 0, st>>>(pt->dev, pr->dev, pr->nrows, pr->nnz, pr->maxrow, pr->d_indptr, pr->d_indices);
        else k_pair_pattern<3><<<grid, block, 0, st>>>(pt->dev, pr->dev, pr->nrows, pr->nnz, pr->maxrow, pr->d_indptr, pr->d_indices);
        IGX_HIP(hipGetLastError());
        IGX_HIP(hipStreamSynchronize(st));
        pr->have_pattern = true;
    }
    if (indptr) IGX_HIP(hipMemcpyAsync(indptr, pr->d_indptr, (size_t)(pr->nrows + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (indices) IGX_HIP(hipMemcpyAsync(indices, pr->d_indices, (size_t)pr->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_pair_assemble(igx_pair *pr, int kind, double *data_out)
{
    if (!pr) { set_error("igx_pair_assemble: null pair"); return IGX_ERR_ARG; }
    if (int rc = pair_patch_ok(pr, kind, "igx_pair_assemble")) return rc;
    const long long total = pr->nrows * pr->maxrow;
    if (int rc = pair_launch_fits(total + 127, "igx_pair_assemble")) return rc;
    igx_patch *pt = pr->pt;
    IGX_HIP(hipSetDevice(pt->ctx->device));
    hipStream_t st = pt->ctx->stream;
    if (!pr->d_data && hipMalloc((void **)&pr->d_data, std::max<size_t>(1, (size_t)pr->nnz) * sizeof(double)) != hipSuccess) {
        pr->d_data = nullptr;
        set_error("hipMalloc of %.2f GB for CSR values failed", pr->nnz * 8.0 / 1e9);
        return IGX_ERR_NOMEM;
    }
    if (pt->knobs.poison) IGX_HIP(hipMemsetAsync(pr->d_data, 0xFF, (size_t)pr->nnz * sizeof(double), st));      // every value must be written
    memset(&pr->timing, 0, sizeof(pr->timing));
    pr->timing.algo_used = IGX_ALGO_ENTRYWISE;
    hipEvent_t *ev = pt->ctx->ev;
    IGX_HIP(hipEventRecord(ev[0], st));
    // the fields depend on geometry and coefficients only, not on the spaces: the patch's own (a form given as expressions is
    // materialised by its generated field kernel), computed unless the patch still holds those of this kind
    if (int rc = igx_fields(pt, kind, nullptr, nullptr)) return rc;
    IGX_HIP(hipEventRecord(ev[1], st));
    if (total > 0) {
        dim3 grid((unsigned)((total + 127) / 128)), block(128);
        const PatchDev &pd = pt->dev;
        if (pr->dim == 2) {
            if (kind == IGX_MASS) k_pair_entries_csr<2, IGX_MASS><<<grid, block, 0, st>>>(pd, pr->dev, pt->d_fields, pr->nrows, pr->maxrow, pr->d_data);
            else k_pair_entries_csr<2, IGX_FORM><<<grid, block, 0, st>>>(pd, pr->dev, pt->d_fields, pr->nrows, pr->maxrow, pr->d_data);
        } else {
            if (kind == IGX_MASS) k_pair_entries_csr<3, IGX_MASS><<<grid, block, 0, st>>>(pd, pr->dev, pt->d_fields, pr->nrows, pr->maxrow, pr->d_data);
            else k_pair_entries_csr<3, IGX_FORM><<<grid, block, 0, st>>>(pd, pr->dev, pt->d_fields, pr->nrows, pr->maxrow, pr->d_data);
        }
        IGX_HIP(hipGetLastError());
    }
    IGX_HIP(hipEventRecord(ev[5], st));
    IGX_HIP(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&pr->timing.total_ms, ev[0], ev[5]);
    (void)hipEventElapsedTime(&pr->timing.fields_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&pr->timing.entry_ms, ev[1], ev[5]);
    pr->timing.n_launches = 1;
    if (data_out) {
        IGX_HIP(hipMemcpyAsync(data_out, pr->d_data, (size_t)pr->nnz * sizeof(double), hipMemcpyDeviceToHost, st));
        IGX_HIP(hipStreamSynchronize(st));
    }
    return IGX_OK;
}

int igx_pair_entries(igx_pair *pr, int kind, const size_t *ij, size_t M, double *out)
{
    if (!pr || (M && (!ij || !out))) { set_error("igx_pair_entries: null argument"); return IGX_ERR_ARG; }
    if (int rc = pair_patch_ok(pr, kind, "igx_pair_entries")) return rc;
    if (M == 0) return IGX_OK;
    if (int rc = pair_launch_fits((long long)std::min<size_t>(M, (size_t)1 << 40) + 127, "igx_pair_entries")) return rc;
    igx_patch *pt = pr->pt;
    IGX_HIP(hipSetDevice(pt->ctx->device));
    hipStream_t st = pt->ctx->stream;
    if (pr->ws_cap < M) {
        (void)hipFree(pr->d_ws_ij); (void)hipFree(pr->d_ws_out);
        pr->d_ws_ij = nullptr; pr->d_ws_out = nullptr; pr->ws_cap = 0;
        if (hipMalloc((void **)&pr->d_ws_ij, 2 * M * sizeof(size_t)) != hipSuccess || hipMalloc((void **)&pr->d_ws_out, M * sizeof(double)) != hipSuccess) {
            (void)hipFree(pr->d_ws_ij); pr->d_ws_ij = nullptr; pr->d_ws_out = nullptr;
            set_error("hipMalloc of %.3f GB for index pairs and entry values failed", M * 24.0 / 1e9);
            return IGX_ERR_NOMEM;
        }
        pr->ws_cap = M;
    }
    IGX_HIP(hipMemcpyAsync(pr->d_ws_ij, ij, 2 * M * sizeof(size_t), hipMemcpyHostToDevice, st));
    if (int rc = igx_fields(pt, kind, nullptr, nullptr)) return rc;
    dim3 grid((unsigned)((M + 127) / 128)), block(128);
    const PatchDev &pd = pt->dev;
    if (pr->dim == 2) {
        if (kind == IGX_MASS) k_pair_entries_list<2, IGX_MASS><<<grid, block, 0, st>>>(pd, pr->dev, pt->d_fields, pr->d_ws_ij, M, pr->d_ws_out);
        else k_pair_entries_list<2, IGX_FORM><<<grid, block, 0, st>>>(pd, pr->dev, pt->d_fields, pr->d_ws_ij, M, pr->d_ws_out);
    } else {
        if (kind == IGX_MASS) k_pair_entries_list<3, IGX_MASS><<<grid, block, 0, st>>>(pd, pr->dev, pt->d_fields, pr->d_ws_ij, M, pr->d_ws_out);
        else k_pair_entries_list<3, IGX_FORM><<<grid, block, 0, st>>>(pd, pr->dev, pt->d_fields, pr->d_ws_ij, M, pr->d_ws_out);
    }
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipMemcpyAsync(out, pr->d_ws_out, M * sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

const double *igx_pair_d_data(const igx_pair *pr) { return pr ? pr->d_data : nullptr; }

int igx_pair_last_timing(const igx_pair *pr, igx_timing *t)
{
    if (!pr || !t) { set_error("igx_pair_last_timing: null argument"); return IGX_ERR_ARG; }
    *t = pr->timing;
    return IGX_OK;
}

} // extern "C"
