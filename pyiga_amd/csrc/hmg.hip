// Local multigrid for hierarchical (HB / THB) spline spaces on the device (include/igx.h igx_csr_rap_d, igx_csr_rect_spmv_d,
// igx_hmg_*; host set-up in pyiga_amd/solvers.py).  The hierarchy is the virtual one of the reference's
// local_mg_step: level l holds the active functions up to level l and the deactivated ones of l; its matrix is the Galerkin
// product of the finer one, and its smoother visits only the rows the refinement touched.
//   k_csr_rap        C = P^T A P on a given pattern of C, P given by its transpose alone (column j of P is row j of P^T).  A group
//                    of G lanes owns ONE output entry C[i, j]: its terms are the pairs (a, b), a over the entries (k, w_a) of row i
//                    of P^T and b over the entries (m, w_b) of row j; term t = a * |row j| + b contributes (w_a A[k, m]) w_b, with
//                    A[k, m] found by bisection in row k of A (columns ascending within a row; an absent entry is no term).  Lane
//                    l adds the terms l, l + G, .. in ascending order, then the G partial sums are added by a shuffle tree of
//                    fixed shape and lane 0 stores the value: no atomics, and neither the grid nor the run changes a bit.  An
//                    entry without terms gets exactly 0.0.  An index outside its array makes the entry NaN instead of a read.
//   k_csr_rect_spmv  y = [b +] s M x for a rectangular CSR matrix: the row loop of k_csr_spmv (a group of GW lanes per row, U
//                    batches in flight, shuffle tree), without a dof mask.  It serves P x_c, P^T r, T^T rhs and the residual.
//   The sweeps are k_csr_gs / k_csr_gs_block of multigrid.hip over the row list of a level, the coarsest solve its
//   k_dense_apply (mg_internal.h).  Everything of a cycle goes to one stream; the host reads one number per iteration of a solve.
#include "solve_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace igx;

namespace {

constexpr int NB_RECT_MAX = 8192;        // blocks of one rectangular product (grid-stride over the rows)
constexpr int BLOCK_RED = 1024;          // threads of the one-block reduction

struct Csr {
    const int32_t *ip, *ix;
    const double *v;
    long long nnz;
};

struct RapArgs {
    long long nf, nc;
    Csr A, T;                             // A (nf x nf), T = P^T (nc x nf)
    const int32_t *cip, *cix;
    double *cv;
    long long cnnz;
};

__device__ __forceinline__ bool range_ok(long long k0, long long k1, long long nnz) { return k0 >= 0 && k0 <= k1 && k1 <= nnz; }

template <int G>
__global__ void __launch_bounds__(BLOCK) k_csr_rap(const RapArgs R)
{
    const int lane = threadIdx.x % G;
    const long long ngroups = (long long)gridDim.x * (BLOCK / G);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long e = (long long)blockIdx.x * (BLOCK / G) + threadIdx.x / G; e < R.cnnz; e += ngroups) {
        // the row of entry e: the last i with cip[i] <= e (rows may be empty); i stays inside [0, nc) whatever cip holds
        long long lo = 0, hi = R.nc - 1;
        while (lo < hi) {
            const long long mid = (lo + hi) / 2;
            if (R.cip[mid + 1] > e) hi = mid;
            else lo = mid + 1;
        }
        const long long i = lo, j = R.cix[e];
        double acc = 0.0;
        bool ok = j >= 0 && j < R.nc;
        long long a0 = 0, a1 = 0, b0 = 0, b1 = 0;
        if (ok) {
            a0 = R.T.ip[i]; a1 = R.T.ip[i + 1]; b0 = R.T.ip[j]; b1 = R.T.ip[j + 1];
            ok = range_ok(a0, a1, R.T.nnz) && range_ok(b0, b1, R.T.nnz);
        }
        if (!ok) acc = nan;
        else {
            const long long nb = b1 - b0, T = (a1 - a0) * nb;
            for (long long t = lane; t < T; t += G) {
                const long long a = a0 + t / nb, b = b0 + t % nb;
                const long long k = R.T.ix[a], m = R.T.ix[b];
                if (k < 0 || k >= R.nf || m < 0 || m >= R.nf) { acc += nan; continue; }
                long long r0 = R.A.ip[k], r1 = R.A.ip[k + 1];
                if (!range_ok(r0, r1, R.A.nnz)) { acc += nan; continue; }
                while (r0 < r1) {                      // first position of row k with a column >= m
                    const long long mid = (r0 + r1) / 2;
                    if (R.A.ix[mid] < m) r0 = mid + 1;
                    else r1 = mid;
                }
                if (r0 < R.A.ip[k + 1] && R.A.ix[r0] == m) acc += (R.T.v[a] * R.A.v[r0]) * R.T.v[b];
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, G);
        if (lane == 0) R.cv[e] = acc;
    }
}

template <int GW, int U>
__global__ void __launch_bounds__(BLOCK) k_csr_rect_spmv(long long nrows, long long ncols, const int32_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices, const double *__restrict__ vals,
                                                         long long nnz, const double *__restrict__ x, const double *b, double s, double *y)
{
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW; I < nrows; I += ngroups) {
        const long long k0 = indptr[I], k1 = indptr[I + 1];
        double acc = 0.0;
        if (!range_ok(k0, k1, nnz)) acc = nan;
        else
            for (long long k = k0 + lane; k < k1; k += U * GW) {
                double v[U], xv[U];
                int c[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool in = k + u * GW < k1;
                    v[u] = in ? vals[k + u * GW] : 0.0;
                    c[u] = in ? indices[k + u * GW] : -1;
                    if (in && (c[u] < 0 || c[u] >= ncols)) { c[u] = -1; v[u] = nan; }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) xv[u] = c[u] >= 0 ? x[c[u]] : 1.0;         // (1: a NaN value stays NaN, a padding 0 stays 0)
#pragma unroll
                for (int u = 0; u < U; ++u) acc += v[u] * xv[u];
            }
#pragma unroll
        for (int off = GW / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, GW);
        if (lane == 0) y[I] = (b ? b[I] : 0.0) + s * acc;
    }
}

template <class F>
decltype(auto) with_rect_kernel(int gw, F &&f)
{
    switch (gw) {
    case 64: return f(k_csr_rect_spmv<64, 8>);
    case 32: return f(k_csr_rect_spmv<32, 4>);
    case 16: return f(k_csr_rect_spmv<16, 4>);
    case 8: return f(k_csr_rect_spmv<8, 4>);
    default: return f(k_csr_rect_spmv<4, 4>);
    }
}

// out[0] = sum over the free i of a[i] b[i]: one block, every thread its entries in ascending order, then the fixed tree
__global__ void __launch_bounds__(BLOCK_RED) k_hmg_dot(long long n, const uint8_t *__restrict__ freem, const double *__restrict__ a,
                                                       const double *__restrict__ b, double *out)
{
    __shared__ double sh[BLOCK_RED];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += BLOCK_RED)
        if (freem[i]) s += a[i] * b[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = BLOCK_RED / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// y = free ? x : 0
__global__ void k_hmg_mask(long long n, const uint8_t *freem, const double *x, double *y)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = freem[i] ? x[i] : 0.0;
}

// y = a x + c y
__global__ void k_hmg_axpby(long long n, double a, const double *x, double c, double *y)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = a * x[i] + c * y[i];
}

unsigned blocks_of(long long n) { return (unsigned)std::max<long long>(1, (n + BLOCK - 1) / BLOCK); }

template <class T>
int upload(const T *h, size_t count, T **d)
{
    (void)hipFree(*d);
    *d = nullptr;
    IGX_HIP(hipMalloc((void **)d, std::max<size_t>(1, count) * sizeof(T)));
    if (count) IGX_HIP(hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice));
    return IGX_OK;
}

// a CSR matrix on the device with the longest row (the group width of its products)
struct DevCsr {
    int32_t *ip = nullptr, *ix = nullptr;
    double *v = nullptr;
    long long nrows = 0, ncols = 0, nnz = 0;
    int gw = 4;
    void release() { (void)hipFree(ip); (void)hipFree(ix); (void)hipFree(v); ip = ix = nullptr; v = nullptr; }
};

// the pattern of an nrows x ncols CSR matrix on the host: pointers monotone, columns inside, and (sorted) ascending within a row
bool pattern_ok(long long nrows, long long ncols, const int32_t *ip, const int32_t *ix, bool sorted, const char *what)
{
    if (ip[0] != 0) { set_error("%s: indptr[0] is %d", what, ip[0]); return false; }
    for (long long i = 0; i < nrows; ++i) {
        if (ip[i + 1] < ip[i]) { set_error("%s: indptr decreases at row %lld", what, i); return false; }
        for (long long k = ip[i]; k < ip[i + 1]; ++k) {
            if (ix[k] < 0 || ix[k] >= ncols) { set_error("%s: column %d of row %lld out of range", what, ix[k], i); return false; }
            if (sorted && k > ip[i] && ix[k] <= ix[k - 1]) { set_error("%s: the columns of row %lld are not ascending", what, i); return false; }
        }
    }
    return true;
}

int longest_row(long long nrows, const int32_t *ip)
{
    int m = 0;
    for (long long i = 0; i < nrows; ++i) m = std::max(m, ip[i + 1] - ip[i]);
    return m;
}

int launch_rect(hipStream_t st, const DevCsr &M, const double *x, const double *b, double s, double *y, int max_blocks = 0)
{
    if (M.nrows == 0) return IGX_OK;
    const long long groups = BLOCK / M.gw;
    const long long cap = max_blocks > 0 ? max_blocks : NB_RECT_MAX;
    const unsigned nb = (unsigned)std::min<long long>(cap, (M.nrows + groups - 1) / groups);
    with_rect_kernel(M.gw, [&](auto k) { k<<<nb, BLOCK, 0, st>>>(M.nrows, M.ncols, M.ip, M.ix, M.v, M.nnz, x, b, s, y); });
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

// the group of k_csr_rap from the longest row of P^T: its square bounds the terms of an entry
int rap_group(int tmax) { return (long long)tmax * tmax >= 64 ? 64 : (long long)tmax * tmax >= 8 ? 16 : 4; }

int launch_rap(igx_ctx *ctx, const RapArgs &R, int group, int max_blocks)
{
    if (R.cnnz == 0) return IGX_OK;
    const long long per_block = BLOCK / group;
    const long long cap = max_blocks > 0 ? max_blocks : (long long)std::max(1, ctx->ncu) * 8;
    const unsigned nb = (unsigned)std::min<long long>(cap, (R.cnnz + per_block - 1) / per_block);
    if (group == 64) k_csr_rap<64><<<nb, BLOCK, 0, ctx->stream>>>(R);
    else if (group == 16) k_csr_rap<16><<<nb, BLOCK, 0, ctx->stream>>>(R);
    else k_csr_rap<4><<<nb, BLOCK, 0, ctx->stream>>>(R);
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

struct HmgLevel {
    DevCsr A;
    std::vector<int32_t> h_ip, h_ix;          // the pattern of A on the host (checks of the smoother's colours)
    bool have_pattern = false, have_vals = false;
    // the transfers to the next coarser level: P (n x nc) and P^T
    DevCsr P, T;
    int tmax = 0;
    bool have_transfer = false;
    // the smoother: the rows of the smoothing set sorted by (colour, index)
    int ncol = 0;
    std::vector<int> coff;
    int32_t *d_rows = nullptr;
    int *d_coff = nullptr;
    long long nrows = 0;
    bool one_block = false, have_smoother = false;
    // work vectors of the level: x | b | r, n each
    double *d_work = nullptr;
    double *x() const { return d_work; }
    double *b() const { return d_work + A.nrows; }
    double *r() const { return d_work + 2 * A.nrows; }
    void release()
    {
        A.release(); P.release(); T.release();
        (void)hipFree(d_rows); (void)hipFree(d_coff); (void)hipFree(d_work);
        d_rows = nullptr; d_coff = nullptr; d_work = nullptr;
    }
};

enum { PH_START = 0, PH_SMOOTH, PH_RESIDUAL, PH_TRANSFER, PH_COARSE };
struct Prof {
    hipStream_t st;
    std::vector<hipEvent_t> ev;
    std::vector<int> level, phase;
    int launches = 0;
};

int mark(Prof *pf, int level, int phase)
{
    if (!pf) return IGX_OK;
    hipEvent_t e;
    IGX_HIP(hipEventCreate(&e));
    pf->ev.push_back(e);
    pf->level.push_back(level);
    pf->phase.push_back(phase);
    IGX_HIP(hipEventRecord(e, pf->st));
    return IGX_OK;
}

} // namespace

struct igx_hmg {
    igx_ctx *ctx = nullptr;
    std::vector<HmgLevel> lv;
    // level 0: x[ind[i]] = sum_j inv[i][j] f[ind[j]]
    double *d_inv = nullptr;
    int32_t *d_ind = nullptr;
    int ninv = -1;
    int smoother = IGX_HMG_GS, steps = 2;
    uint8_t *d_free = nullptr;                // 1 on the dofs the residual norm runs over (finest level)
    long long nfree = 0;
    double *d_vec = nullptr;                  // r | z | p | q of a solve, n of the finest level each
    double *d_sc = nullptr;                   // two scalars
};

namespace {

int sweeps(hipStream_t st, igx_hmg *h, HmgLevel &L, double *x, const double *b, bool post, Prof *pf)
{
    int *cnt = pf ? &pf->launches : nullptr;
    auto one = [&](bool backward) {
        return csr_gs_sweep(st, L.A.gw, L.ncol, L.coff.data(), L.d_coff, L.d_rows, L.one_block, L.A.ip, L.A.ix, L.A.v, x, b, backward, cnt);
    };
    if (L.nrows == 0) return IGX_OK;
    for (int k = 0; k < h->steps; ++k) {
        int rc = IGX_OK;
        switch (h->smoother) {
        case IGX_HMG_GS: rc = one(post); break;
        case IGX_HMG_FORWARD_GS: rc = one(false); break;
        case IGX_HMG_BACKWARD_GS: rc = one(true); break;
        default: rc = one(false); if (!rc) rc = one(true); break;
        }
        if (rc) return rc;
    }
    return IGX_OK;
}

// x <- one cycle on level l with the right-hand side f (the reference's step)
int cycle(hipStream_t st, igx_hmg *h, int l, const double *f, double *x, Prof *pf)
{
    HmgLevel &L = h->lv[l];
    if (l == 0) {
        if (int rc = dense_apply(st, h->ninv, h->d_inv, h->d_ind, f, x)) return rc;
        if (pf) ++pf->launches;
        return mark(pf, 0, PH_COARSE);
    }
    HmgLevel &C = h->lv[l - 1];
    if (int rc = sweeps(st, h, L, x, f, false, pf)) return rc;
    if (int rc = mark(pf, l, PH_SMOOTH)) return rc;
    if (int rc = launch_rect(st, L.A, x, f, -1.0, L.r())) return rc;            // r = f - A x, every row
    if (int rc = mark(pf, l, PH_RESIDUAL)) return rc;
    if (int rc = launch_rect(st, L.T, L.r(), nullptr, 1.0, C.b())) return rc;   // r_c = P^T r
    IGX_HIP(hipMemsetAsync(C.x(), 0, (size_t)C.A.nrows * sizeof(double), st));
    if (int rc = mark(pf, l, PH_TRANSFER)) return rc;
    if (int rc = cycle(st, h, l - 1, C.b(), C.x(), pf)) return rc;
    if (int rc = launch_rect(st, L.P, C.x(), x, 1.0, x)) return rc;             // x += P e
    if (int rc = mark(pf, l, PH_TRANSFER)) return rc;
    if (int rc = sweeps(st, h, L, x, f, true, pf)) return rc;
    if (pf) pf->launches += 3;
    return mark(pf, l, PH_SMOOTH);
}

int hmg_ready(const igx_hmg *h, const char *what)
{
    if (!h) { set_error("%s: null handle", what); return IGX_ERR_ARG; }
    const int L = (int)h->lv.size();
    for (int l = 0; l < L; ++l) {
        const HmgLevel &V = h->lv[l];
        if (!V.have_pattern || !V.have_vals) { set_error("%s: level %d has no matrix (igx_hmg_set_matrix / igx_hmg_galerkin)", what, l); return IGX_ERR_ARG; }
        if (l == 0) continue;
        if (!V.have_transfer) { set_error("%s: level %d has no prolongation (igx_hmg_set_transfer)", what, l); return IGX_ERR_ARG; }
        if (!V.have_smoother) { set_error("%s: level %d has no smoothing set (igx_hmg_set_smoother)", what, l); return IGX_ERR_ARG; }
        if (V.P.ncols != h->lv[l - 1].A.nrows) { set_error("%s: the prolongation of level %d has %lld columns, level %d %lld rows", what, l, V.P.ncols, l - 1, h->lv[l - 1].A.nrows); return IGX_ERR_ARG; }
    }
    if (h->ninv < 0) { set_error("%s: level 0 has no inverse (igx_hmg_set_inverse)", what); return IGX_ERR_ARG; }
    if (!h->d_free) { set_error("%s: the dofs of the residual norm are not set (igx_hmg_set_free)", what); return IGX_ERR_ARG; }
    return IGX_OK;
}

HmgLevel *level_arg(igx_hmg *h, int level, const char *what)
{
    if (!h) { set_error("%s: null handle", what); return nullptr; }
    if (level < 0 || level >= (int)h->lv.size()) { set_error("%s: level %d of %d", what, level, (int)h->lv.size()); return nullptr; }
    return &h->lv[level];
}

int set_csr(DevCsr &M, long long nrows, long long ncols, const int32_t *ip, const int32_t *ix, const double *vals_host)
{
    M.nrows = nrows; M.ncols = ncols; M.nnz = ip[nrows];
    M.gw = spmv_group_width(longest_row(nrows, ip));
    if (int rc = upload(ip, (size_t)nrows + 1, &M.ip)) return rc;
    if (int rc = upload(ix, (size_t)M.nnz, &M.ix)) return rc;
    if (vals_host) return upload(vals_host, (size_t)M.nnz, &M.v);
    (void)hipFree(M.v);
    M.v = nullptr;
    IGX_HIP(hipMalloc((void **)&M.v, std::max<size_t>(1, (size_t)M.nnz) * sizeof(double)));
    return IGX_OK;
}

double read_scalar(hipStream_t st, const double *d, int *rc)
{
    double v = 0.0;
    const hipError_t e = hipMemcpyAsync(&v, d, sizeof(double), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(st) : e;
    if (e2 != hipSuccess) { set_error("igx_hmg_solve_d: %s", hipGetErrorString(e2)); *rc = IGX_ERR_HIP; }
    return v;
}

} // namespace

extern "C" {

int igx_csr_rap_d(igx_ctx *ctx, int64_t n_f, int64_t n_c, const int32_t *d_a_indptr, const int32_t *d_a_indices, const double *d_a_vals,
                  int64_t a_nnz, const int32_t *d_pt_indptr, const int32_t *d_pt_indices, const double *d_pt_vals, int64_t pt_nnz,
                  int32_t pt_row_max, const int32_t *d_c_indptr, const int32_t *d_c_indices, double *d_c_vals, int64_t c_nnz,
                  int32_t max_blocks)
{
    const char *what = "igx_csr_rap_d";
    if (!ctx) { set_error("%s: null context", what); return IGX_ERR_ARG; }
    if (n_f < 0 || n_c < 0 || a_nnz < 0 || pt_nnz < 0 || c_nnz < 0 || pt_row_max < 0 || max_blocks < 0) { set_error("%s: negative size", what); return IGX_ERR_ARG; }
    if (c_nnz == 0) return IGX_OK;
    if (n_c == 0) { set_error("%s: %lld values of a matrix without rows", what, (long long)c_nnz); return IGX_ERR_ARG; }
    if (!d_a_indptr || !d_pt_indptr || !d_c_indptr || !d_c_indices || !d_c_vals || (a_nnz && (!d_a_indices || !d_a_vals)) ||
        (pt_nnz && (!d_pt_indices || !d_pt_vals))) {
        set_error("%s: null device pointer", what); return IGX_ERR_ARG;
    }
    IGX_HIP(hipSetDevice(ctx->device));
    RapArgs R{n_f, n_c, Csr{d_a_indptr, d_a_indices, d_a_vals, a_nnz}, Csr{d_pt_indptr, d_pt_indices, d_pt_vals, pt_nnz}, d_c_indptr,
              d_c_indices, d_c_vals, c_nnz};
    return launch_rap(ctx, R, rap_group(pt_row_max), max_blocks);
}

int igx_csr_rect_spmv_d(igx_ctx *ctx, int64_t nrows, int64_t ncols, const int32_t *d_indptr, const int32_t *d_indices, const double *d_vals,
                        int64_t nnz, int32_t row_max, const double *d_x, double *d_y, int accumulate, int32_t max_blocks)
{
    const char *what = "igx_csr_rect_spmv_d";
    if (!ctx) { set_error("%s: null context", what); return IGX_ERR_ARG; }
    if (nrows < 0 || ncols < 0 || nnz < 0 || row_max < 0 || max_blocks < 0) { set_error("%s: negative size", what); return IGX_ERR_ARG; }
    if (nrows == 0) return IGX_OK;
    if (!d_indptr || !d_y || (nnz && (!d_indices || !d_vals || !d_x)) || d_x == d_y) { set_error("%s: null device pointer, or x is y", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(ctx->device));
    DevCsr M;
    M.ip = const_cast<int32_t *>(d_indptr); M.ix = const_cast<int32_t *>(d_indices); M.v = const_cast<double *>(d_vals);
    M.nrows = nrows; M.ncols = ncols; M.nnz = nnz; M.gw = spmv_group_width(row_max);
    return launch_rect(ctx->stream, M, d_x, accumulate ? d_y : nullptr, 1.0, d_y, max_blocks);
}

int igx_hmg_create(igx_ctx *ctx, int nlevels, igx_hmg **out)
{
    if (out) *out = nullptr;
    if (!ctx || !out || nlevels < 1 || nlevels > IGX_HMG_MAX_LEVELS) { set_error("igx_hmg_create: null argument, or %d levels (1 .. %d)", nlevels, IGX_HMG_MAX_LEVELS); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(ctx->device));
    igx_hmg *h = new igx_hmg;
    h->ctx = ctx;
    h->lv.resize((size_t)nlevels);
    if (hipMalloc((void **)&h->d_sc, 2 * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        set_error("igx_hmg_create: out of device memory");
        return IGX_ERR_NOMEM;
    }
    *out = h;
    return IGX_OK;
}

void igx_hmg_destroy(igx_hmg *h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    for (HmgLevel &L : h->lv) L.release();
    (void)hipFree(h->d_inv); (void)hipFree(h->d_ind); (void)hipFree(h->d_free); (void)hipFree(h->d_vec); (void)hipFree(h->d_sc);
    delete h;
}

int igx_hmg_set_matrix(igx_hmg *h, int level, int64_t n, const int32_t *indptr, const int32_t *indices, const double *d_vals)
{
    const char *what = "igx_hmg_set_matrix";
    HmgLevel *L = level_arg(h, level, what);
    if (!L) return IGX_ERR_ARG;
    if (n < 0 || !indptr || (indptr[n] > 0 && !indices)) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    if (!pattern_ok(n, n, indptr, indices, true, what)) return IGX_ERR_ARG;
    IGX_HIP(hipSetDevice(h->ctx->device));
    IGX_HIP(hipStreamSynchronize(h->ctx->stream));
    L->have_pattern = L->have_vals = L->have_smoother = false;
    if (int rc = set_csr(L->A, n, n, indptr, indices, nullptr)) return rc;
    L->h_ip.assign(indptr, indptr + n + 1);
    L->h_ix.assign(indices, indices + indptr[n]);
    (void)hipFree(L->d_work);
    L->d_work = nullptr;
    IGX_HIP(hipMalloc((void **)&L->d_work, std::max<size_t>(1, 3 * (size_t)n) * sizeof(double)));
    IGX_HIP(hipMemset(L->d_work, 0, std::max<size_t>(1, 3 * (size_t)n) * sizeof(double)));
    L->have_pattern = true;
    if (d_vals) {
        if (L->A.nnz) IGX_HIP(hipMemcpy(L->A.v, d_vals, (size_t)L->A.nnz * sizeof(double), hipMemcpyDeviceToDevice));
        L->have_vals = true;
    }
    if (level == (int)h->lv.size() - 1) {         // the vectors of a solve follow the finest level
        (void)hipFree(h->d_vec); (void)hipFree(h->d_free);
        h->d_vec = nullptr; h->d_free = nullptr;
        IGX_HIP(hipMalloc((void **)&h->d_vec, std::max<size_t>(1, 4 * (size_t)n) * sizeof(double)));
    }
    return IGX_OK;
}

int igx_hmg_set_transfer(igx_hmg *h, int level, int64_t n_c, const int32_t *indptr, const int32_t *indices, const double *vals)
{
    const char *what = "igx_hmg_set_transfer";
    HmgLevel *L = level_arg(h, level, what);
    if (!L) return IGX_ERR_ARG;
    if (level == 0) { set_error("%s: level 0 has no coarser level", what); return IGX_ERR_ARG; }
    if (!L->have_pattern) { set_error("%s: level %d has no matrix yet", what, level); return IGX_ERR_ARG; }
    const long long n = L->A.nrows;
    if (n_c < 0 || !indptr || (indptr[n] > 0 && (!indices || !vals))) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    if (!pattern_ok(n, n_c, indptr, indices, false, what)) return IGX_ERR_ARG;
    // the transpose, rows in ascending column order of P: entries of a row of P^T ascend with the row of P they came from
    const long long nnz = indptr[n];
    std::vector<int32_t> tip((size_t)n_c + 1, 0), tix((size_t)nnz);
    std::vector<double> tv((size_t)nnz);
    for (long long k = 0; k < nnz; ++k) ++tip[(size_t)indices[k] + 1];
    for (long long j = 0; j < n_c; ++j) tip[j + 1] += tip[j];
    {
        std::vector<int32_t> at(tip.begin(), tip.end() - 1);
        for (long long i = 0; i < n; ++i)
            for (long long k = indptr[i]; k < indptr[i + 1]; ++k) {
                const int32_t q = at[indices[k]]++;
                tix[q] = (int32_t)i;
                tv[q] = vals[k];
            }
    }
    IGX_HIP(hipSetDevice(h->ctx->device));
    IGX_HIP(hipStreamSynchronize(h->ctx->stream));
    L->have_transfer = false;
    if (int rc = set_csr(L->P, n, n_c, indptr, indices, vals)) return rc;
    if (int rc = set_csr(L->T, n_c, n, tip.data(), tix.data(), tv.data())) return rc;
    L->tmax = longest_row(n_c, tip.data());
    L->have_transfer = true;
    return IGX_OK;
}

int igx_hmg_galerkin(igx_hmg *h, int level, int32_t max_blocks)
{
    const char *what = "igx_hmg_galerkin";
    HmgLevel *L = level_arg(h, level, what);
    if (!L) return IGX_ERR_ARG;
    if (level == 0 || max_blocks < 0) { set_error("%s: level 0 has no coarser level, or a negative cap", what); return IGX_ERR_ARG; }
    HmgLevel &C = h->lv[level - 1];
    if (!L->have_vals || !L->have_transfer || !C.have_pattern) { set_error("%s: level %d needs its matrix and prolongation, level %d its pattern", what, level, level - 1); return IGX_ERR_ARG; }
    if (L->P.ncols != C.A.nrows) { set_error("%s: the prolongation has %lld columns, level %d %lld rows", what, L->P.ncols, level - 1, C.A.nrows); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(h->ctx->device));
    RapArgs R{L->A.nrows, C.A.nrows, Csr{L->A.ip, L->A.ix, L->A.v, L->A.nnz}, Csr{L->T.ip, L->T.ix, L->T.v, L->T.nnz}, C.A.ip, C.A.ix, C.A.v, C.A.nnz};
    if (int rc = launch_rap(h->ctx, R, rap_group(L->tmax), max_blocks)) return rc;
    C.have_vals = true;
    return IGX_OK;
}

int igx_hmg_set_smoother(igx_hmg *h, int level, int32_t ncolours, const int32_t *colour_offsets, const int32_t *rows, int64_t block_rows)
{
    const char *what = "igx_hmg_set_smoother";
    HmgLevel *L = level_arg(h, level, what);
    if (!L) return IGX_ERR_ARG;
    if (!L->have_pattern) { set_error("%s: level %d has no matrix yet", what, level); return IGX_ERR_ARG; }
    if (ncolours < 0 || !colour_offsets || colour_offsets[0] != 0) { set_error("%s: bad colour offsets", what); return IGX_ERR_ARG; }
    const long long n = L->A.nrows, nr = colour_offsets[ncolours];
    if (nr > 0 && !rows) { set_error("%s: null rows", what); return IGX_ERR_ARG; }
    std::vector<int32_t> colour((size_t)n, -1);
    for (int c = 0; c < ncolours; ++c) {
        if (colour_offsets[c + 1] < colour_offsets[c]) { set_error("%s: colour offsets decrease", what); return IGX_ERR_ARG; }
        for (long long k = colour_offsets[c]; k < colour_offsets[c + 1]; ++k) {
            const int32_t i = rows[k];
            if (i < 0 || i >= n) { set_error("%s: row %d out of range", what, i); return IGX_ERR_ARG; }
            if (colour[i] >= 0) { set_error("%s: row %d is listed twice", what, i); return IGX_ERR_ARG; }
            colour[i] = c;
        }
    }
    // rows of one colour are relaxed at once: they must not couple, in either orientation
    for (long long i = 0; i < n; ++i)
        for (long long k = L->h_ip[i]; k < L->h_ip[i + 1]; ++k) {
            const int32_t j = L->h_ix[k];
            if (j != i && colour[i] >= 0 && colour[j] == colour[i]) {
                set_error("%s: rows %lld and %d are coupled and both have colour %d", what, i, j, colour[i]);
                return IGX_ERR_ARG;
            }
        }
    IGX_HIP(hipSetDevice(h->ctx->device));
    IGX_HIP(hipStreamSynchronize(h->ctx->stream));
    L->have_smoother = false;
    if (int rc = upload(rows, (size_t)nr, &L->d_rows)) return rc;
    L->coff.assign(colour_offsets, colour_offsets + ncolours + 1);
    if (int rc = upload(L->coff.data(), L->coff.size(), &L->d_coff)) return rc;
    L->ncol = ncolours;
    L->nrows = nr;
    L->one_block = nr <= block_rows;
    L->have_smoother = true;
    return IGX_OK;
}

int igx_hmg_set_inverse(igx_hmg *h, const int32_t *ind, int64_t m, const double *inv)
{
    const char *what = "igx_hmg_set_inverse";
    HmgLevel *L = level_arg(h, 0, what);
    if (!L) return IGX_ERR_ARG;
    if (!L->have_pattern) { set_error("%s: level 0 has no matrix yet", what); return IGX_ERR_ARG; }
    if (m < 0 || m > 8192 || (m > 0 && (!ind || !inv))) { set_error("%s: null argument, or %lld rows (at most 8192)", what, (long long)m); return IGX_ERR_ARG; }
    for (long long k = 0; k < m; ++k)
        if (ind[k] < 0 || ind[k] >= L->A.nrows) { set_error("%s: index %d out of range", what, ind[k]); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(h->ctx->device));
    IGX_HIP(hipStreamSynchronize(h->ctx->stream));
    h->ninv = -1;
    if (int rc = upload(ind, (size_t)m, &h->d_ind)) return rc;
    if (int rc = upload(inv, (size_t)m * (size_t)m, &h->d_inv)) return rc;
    h->ninv = (int)m;
    return IGX_OK;
}

int igx_hmg_set_options(igx_hmg *h, int smoother, int smooth_steps)
{
    if (!h || smoother < IGX_HMG_GS || smoother > IGX_HMG_SYMMETRIC_GS || smooth_steps < 1 || smooth_steps > 16) {
        set_error("igx_hmg_set_options: null handle, unknown smoother %d, or %d smoothing steps (1 .. 16)", smoother, smooth_steps);
        return IGX_ERR_ARG;
    }
    h->smoother = smoother;
    h->steps = smooth_steps;
    return IGX_OK;
}

int igx_hmg_set_free(igx_hmg *h, const uint8_t *free_mask)
{
    const char *what = "igx_hmg_set_free";
    if (!h || !free_mask) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    const HmgLevel &L = h->lv.back();
    if (!L.have_pattern) { set_error("%s: the finest level has no matrix yet", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(h->ctx->device));
    IGX_HIP(hipStreamSynchronize(h->ctx->stream));
    h->nfree = 0;
    for (long long i = 0; i < L.A.nrows; ++i) h->nfree += free_mask[i] ? 1 : 0;
    return upload(free_mask, (size_t)L.A.nrows, &h->d_free);
}

int igx_hmg_level_values(igx_hmg *h, int level, double *out)
{
    const char *what = "igx_hmg_level_values";
    HmgLevel *L = level_arg(h, level, what);
    if (!L) return IGX_ERR_ARG;
    if (!out || !L->have_vals) { set_error("%s: null argument, or level %d has no values", what, level); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(h->ctx->device));
    IGX_HIP(hipStreamSynchronize(h->ctx->stream));
    if (L->A.nnz) IGX_HIP(hipMemcpy(out, L->A.v, (size_t)L->A.nnz * sizeof(double), hipMemcpyDeviceToHost));
    return IGX_OK;
}

int igx_hmg_spmv_d(igx_hmg *h, const double *d_x, const double *d_b, double sign, double *d_y)
{
    const char *what = "igx_hmg_spmv_d";
    if (!h || !d_x || !d_y || d_x == d_y) { set_error("%s: null argument, or x is y", what); return IGX_ERR_ARG; }
    const HmgLevel &L = h->lv.back();
    if (!L.have_vals) { set_error("%s: the finest level has no matrix", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(h->ctx->device));
    return launch_rect(h->ctx->stream, L.A, d_x, d_b, sign, d_y);
}

int igx_hmg_cycle_d(igx_hmg *h, const double *d_f, double *d_x)
{
    const char *what = "igx_hmg_cycle_d";
    if (int rc = hmg_ready(h, what)) return rc;
    if (!d_f || !d_x || d_f == d_x) { set_error("%s: null argument, or f is x", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(h->ctx->device));
    return cycle(h->ctx->stream, h, (int)h->lv.size() - 1, d_f, d_x, nullptr);
}

int igx_hmg_solve_d(igx_hmg *h, int method, const double *d_f, double *d_x, double tol, int maxiter, igx_hmg_info *info)
{
    const char *what = "igx_hmg_solve_d";
    if (int rc = hmg_ready(h, what)) return rc;
    if (!d_f || !d_x || d_f == d_x || !info || !(tol > 0.0) || maxiter < 1) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    if (method != IGX_HMG_ITERATE && method != IGX_HMG_CG) { set_error("%s: unknown method %d", what, method); return IGX_ERR_ARG; }
    if (method == IGX_HMG_CG && h->smoother != IGX_HMG_GS && h->smoother != IGX_HMG_SYMMETRIC_GS) {
        set_error("%s: CG needs a symmetric cycle (gs or symmetric_gs)", what);
        return IGX_ERR_UNSUPPORTED;
    }
    std::memset(info, 0, sizeof(*info));
    info->n_free = h->nfree;
    IGX_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int top = (int)h->lv.size() - 1;
    const HmgLevel &L = h->lv[top];
    const long long n = L.A.nrows;
    double *r = h->d_vec, *z = r + n, *p = z + n, *q = p + n;
    const unsigned nbv = blocks_of(n);
    int rc = IGX_OK;
    auto norm2 = [&](const double *a, const double *b) {       // sum over the free dofs of a b
        k_hmg_dot<<<1, BLOCK_RED, 0, st>>>(n, h->d_free, a, b, h->d_sc);
        return read_scalar(st, h->d_sc, &rc);
    };
    IGX_HIP(hipMemsetAsync(d_x, 0, (size_t)n * sizeof(double), st));
    const double res0 = std::sqrt(norm2(d_f, d_f));
    if (rc) return rc;
    if (!(res0 > 0.0)) { info->converged = 1; return IGX_OK; }              // (f vanishes on the free dofs: x = 0)
    if (method == IGX_HMG_ITERATE) {
        for (int it = 1; it <= maxiter; ++it) {
            if ((rc = cycle(st, h, top, d_f, d_x, nullptr))) return rc;
            if ((rc = launch_rect(st, L.A, d_x, d_f, -1.0, r))) return rc;
            const double res = std::sqrt(norm2(r, r));
            if (rc) return rc;
            info->iterations = it;
            info->ratio = res / res0;
            if (info->ratio < tol) { info->converged = 1; break; }
            if (!std::isfinite(info->ratio)) break;
        }
        return IGX_OK;
    }
    // CG on the free dofs, z = B r: one cycle from a zero guess (B is symmetric for gs and symmetric_gs)
    auto precond = [&]() -> int {
        IGX_HIP(hipMemsetAsync(z, 0, (size_t)n * sizeof(double), st));
        if (int e = cycle(st, h, top, r, z, nullptr)) return e;
        k_hmg_mask<<<nbv, BLOCK, 0, st>>>(n, h->d_free, z, z);
        IGX_HIP(hipGetLastError());
        return IGX_OK;
    };
    k_hmg_mask<<<nbv, BLOCK, 0, st>>>(n, h->d_free, d_f, r);
    IGX_HIP(hipGetLastError());
    if ((rc = precond())) return rc;
    IGX_HIP(hipMemcpyAsync(p, z, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    double rz = norm2(r, z);
    if (rc) return rc;
    for (int it = 1; it <= maxiter; ++it) {
        if ((rc = launch_rect(st, L.A, p, nullptr, 1.0, q))) return rc;
        const double pq = norm2(p, q);                           // (the free rows of q only: q needs no mask)
        if (rc) return rc;
        if (!(pq > 0.0) || !(rz > 0.0)) break;                  // not positive definite (or converged to the last bit)
        const double alpha = rz / pq;
        k_hmg_axpby<<<nbv, BLOCK, 0, st>>>(n, alpha, p, 1.0, d_x);
        k_hmg_axpby<<<nbv, BLOCK, 0, st>>>(n, -alpha, q, 1.0, r);
        k_hmg_mask<<<nbv, BLOCK, 0, st>>>(n, h->d_free, r, r);
        IGX_HIP(hipGetLastError());
        const double res = std::sqrt(norm2(r, r));
        if (rc) return rc;
        info->iterations = it;
        info->ratio = res / res0;
        if (info->ratio < tol) { info->converged = 1; break; }
        if (!std::isfinite(info->ratio)) break;
        if ((rc = precond())) return rc;
        const double rz1 = norm2(r, z);
        if (rc) return rc;
        k_hmg_axpby<<<nbv, BLOCK, 0, st>>>(n, 1.0, z, rz1 / rz, p);
        IGX_HIP(hipGetLastError());
        rz = rz1;
    }
    return IGX_OK;
}

int igx_hmg_profile_d(igx_hmg *h, const double *d_f, double *d_x, int reps, igx_hmg_profile *out)
{
    const char *what = "igx_hmg_profile_d";
    if (int rc = hmg_ready(h, what)) return rc;
    if (!d_f || !d_x || d_f == d_x || !out || reps < 1) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    std::memset(out, 0, sizeof(*out));
    out->levels = (int32_t)h->lv.size();
    for (int rep = 0; rep < reps; ++rep) {
        Prof pf;
        pf.st = st;
        int rc = mark(&pf, 0, PH_START);
        if (!rc) rc = cycle(st, h, (int)h->lv.size() - 1, d_f, d_x, &pf);
        const hipError_t e = hipStreamSynchronize(st);
        if (!rc && e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); rc = IGX_ERR_HIP; }
        for (size_t k = 1; !rc && k < pf.ev.size(); ++k) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, pf.ev[k - 1], pf.ev[k]);
            const int l = pf.level[k];
            out->total_ms += ms;
            switch (pf.phase[k]) {
            case PH_SMOOTH: out->smooth_ms[l] += ms; break;
            case PH_RESIDUAL: out->residual_ms[l] += ms; break;
            case PH_TRANSFER: out->transfer_ms[l] += ms; break;
            default: out->coarse_ms += ms; break;
            }
        }
        for (hipEvent_t ev : pf.ev) (void)hipEventDestroy(ev);
        if (rc) return rc;
        out->launches = pf.launches;
    }
    const float inv = 1.0f / (float)reps;
    out->total_ms *= inv; out->coarse_ms *= inv;
    for (int l = 0; l < IGX_HMG_MAX_LEVELS; ++l) { out->smooth_ms[l] *= inv; out->residual_ms[l] *= inv; out->transfer_ms[l] *= inv; }
    return IGX_OK;
}

int igx_hmg_level_info(igx_hmg *h, int level, igx_hmg_level *out)
{
    const char *what = "igx_hmg_level_info";
    HmgLevel *L = level_arg(h, level, what);
    if (!L || !out) { if (L) set_error("%s: null argument", what); return IGX_ERR_ARG; }
    std::memset(out, 0, sizeof(*out));
    out->nrows = L->A.nrows;
    out->nnz = L->A.nnz;
    out->nsmooth = level == 0 ? std::max(h->ninv, 0) : L->nrows;
    out->ncolours = L->ncol;
    out->one_block = L->one_block ? 1 : 0;
    out->group_width = L->A.gw;
    return IGX_OK;
}

} // extern "C"
