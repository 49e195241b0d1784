// Geometric multigrid as the preconditioner of a multipatch solver (igx_solver_set_mg_*, igx_solver_mg_*; include/igx.h,
// DESIGN.md section 17).  A hierarchy is a chain of multipatch solvers, each over the sums of the same problem on a coarser
// space; every solver carries its level (MgLevel): the smoother's colour lists, the transfers to the next coarser solver, or the
// dense inverse of the coarsest matrix.
//   k_csr_gs        one colour of a Gauss-Seidel sweep over the multipatch CSR: the row loop of k_csr_spmv (one group of GW lanes
//                   per row, values and indices streamed once, x gathered through the caches) over the rows of the colour; the
//                   group leader writes x[i] = (b[i] - sum_{j != i} a_ij x_j) / a_ii.  Rows of one colour never couple, so one
//                   launch per colour in stream order is the sequential sweep in (colour, index) order.
//   k_csr_gs_block  the whole sweep of a small level in one block of 1024 threads: the colours one after the other,
//                   __syncthreads() in between.
//   k_mg_transfer   prolongation and restriction of one patch: every local dof of the target space contracts the banded 1D
//                   matrices P_0 (x) P_1 (x) P_2 (their transposes) against the source vector, read through the patch's
//                   local-to-global map, and stores (prolongation: shared dofs get the same value from every patch) or adds
//                   (restriction) at its global dof.  One launch per patch, in patch order: the result is deterministic.
//   k_dense_apply   the coarsest level: x = A_c^-1 b with the dense inverse, one block per row, fixed summation tree.
// A multipatch block solver (a vector-valued form, nc components) hangs the same levels on the same chain
// through igx_solver_set_block_mg_*: its smoother relaxes nodes (scalar dofs with their nc components: csr_node_gs_sweep of
// multigrid_block.hip), its transfers are k_mg_transfer launched per patch and component on that component's slice of the
// vectors and of the mask, its dense inverse acts on the blocked free dofs.
// The colouring itself (igx_csr_colouring: first fit in ascending dof order) is host code and needs no device.
#include "mg_internal.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace igx;

namespace {

constexpr int BLOCK = 256;
constexpr int NB_GS_MAX = 8192;          // blocks of one colour's launch (grid-stride over the rows of the colour)
constexpr int BLOCK_ONE = 1024;          // threads of the one-block sweep: its row groups are all the parallelism a colour gets

// one Gauss-Seidel row by a group of GW lanes: U batches of GW values per lane in flight, as k_csr_spmv
template <int GW, int U>
__device__ __forceinline__ void gs_row(long long I, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                       const double *__restrict__ vals, double *x, const double *__restrict__ b, int lane)
{
    const long long k0 = indptr[I], k1 = indptr[I + 1];
    double acc = 0.0, dg = 0.0;
    for (long long k = k0 + lane; k < k1; k += U * GW) {
        double v[U], xv[U];
        int c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = k + u * GW < k1;
            v[u] = in ? __builtin_nontemporal_load(vals + k + u * GW) : 0.0;
            c[u] = in ? __builtin_nontemporal_load(indices + k + u * GW) : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = (c[u] >= 0 && c[u] != I) ? x[c[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            acc += v[u] * xv[u];
            if (c[u] == I) dg += v[u];
        }
    }
#pragma unroll
    for (int off = GW / 2; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off, GW);
        dg += __shfl_xor(dg, off, GW);
    }
    if (lane == 0 && dg != 0.0) x[I] = (b[I] - acc) / dg;          // (a zero diagonal leaves x[I])
}

// the rows rows[0 .. nr) of one colour
template <int GW, int U>
__global__ void __launch_bounds__(BLOCK) k_csr_gs(long long nr, const int32_t *__restrict__ rows, const int32_t *__restrict__ indptr,
                                                  const int32_t *__restrict__ indices, const double *__restrict__ vals, double *x,
                                                  const double *__restrict__ b)
{
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    for (long long r = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW; r < nr; r += ngroups)
        gs_row<GW, U>(rows[r], indptr, indices, vals, x, b, lane);
}

// every colour of a sweep in one block: colour c holds rows[coff[c] .. coff[c + 1]); backward: the colours in descending order
template <int GW, int U>
__global__ void __launch_bounds__(BLOCK_ONE) k_csr_gs_block(int ncol, const int *__restrict__ coff, const int32_t *__restrict__ rows,
                                                        const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                        const double *__restrict__ vals, double *x, const double *__restrict__ b,
                                                        int backward)
{
    const int lane = threadIdx.x % GW, group = threadIdx.x / GW;
    for (int ci = 0; ci < ncol; ++ci) {
        const int c = backward ? ncol - 1 - ci : ci;
        const int r1 = coff[c + 1];
        for (int r = coff[c] + group; r < r1; r += BLOCK_ONE / GW) gs_row<GW, U>(rows[r], indptr, indices, vals, x, b, lane);
        __syncthreads();                             // (the block's writes to x are visible to its next colour)
    }
}

// f(the sweep kernels at group width gw): the widths and batches of the CSR SpMV
template <class F>
decltype(auto) with_gs_kernel(int gw, F &&f)
{
    switch (gw) {
    case 64: return f(k_csr_gs<64, 8>, k_csr_gs_block<64, 8>);
    case 32: return f(k_csr_gs<32, 4>, k_csr_gs_block<32, 4>);
    case 16: return f(k_csr_gs<16, 4>, k_csr_gs_block<16, 4>);
    case 8: return f(k_csr_gs<8, 4>, k_csr_gs_block<8, 4>);
    default: return f(k_csr_gs<4, 4>, k_csr_gs_block<4, 4>);
    }
}

// one patch's transfer: the target's local dofs (No, 3D; a 2D patch has a one-dof outer axis) from the source's (Ni).  Axis k of
// target index i reads the source indices lo[k][i] .. lo[k][i] + w[k] with the weights v[k][i * w[k] ..] (zero-padded; lo + w <= Ni)
struct Transfer {
    int No[3], Ni[3], w[3];
    const int *lo[3];
    const double *v[3];
    const int32_t *l2g_o, *l2g_i;
    long long nout;
};

// ADD: out[g] += acc on the free g (restriction; the map of a patch is injective: no two entries of one pass meet), else
// out[g] = free[g] ? acc : 0 (prolongation).  scale: a factor per source dof (1 / multiplicity), or null
template <bool ADD>
__global__ void __launch_bounds__(BLOCK) k_mg_transfer(const Transfer T, const uint8_t *__restrict__ free_o, const double *__restrict__ scale,
                                                       const double *__restrict__ in, double *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.nout) return;
    const int g = T.l2g_o[i];
    if (!free_o[g]) {
        if (!ADD) out[g] = 0.0;
        return;
    }
    const int i2 = (int)(i % T.No[2]);
    const long long t = i / T.No[2];
    const int i1 = (int)(t % T.No[1]), i0 = (int)(t / T.No[1]);
    const int l0 = T.lo[0][i0], l1 = T.lo[1][i1], l2 = T.lo[2][i2];
    double acc = 0.0;
    for (int t0 = 0; t0 < T.w[0]; ++t0) {
        const double a0 = T.v[0][i0 * T.w[0] + t0];
        if (a0 == 0.0) continue;
        for (int t1 = 0; t1 < T.w[1]; ++t1) {
            const double a1 = a0 * T.v[1][i1 * T.w[1] + t1];
            if (a1 == 0.0) continue;
            const long long base = ((long long)(l0 + t0) * T.Ni[1] + (l1 + t1)) * T.Ni[2] + l2;
            for (int t2 = 0; t2 < T.w[2]; ++t2) {
                const double a2 = T.v[2][i2 * T.w[2] + t2];
                if (a2 == 0.0) continue;
                const int gi = T.l2g_i[base + t2];
                const double xv = scale ? scale[gi] * in[gi] : in[gi];
                acc += a1 * a2 * xv;
            }
        }
    }
    if (ADD) out[g] += acc;
    else out[g] = acc;
}

// x[fr[i]] = sum_j inv[i][j] b[fr[j]]: one block per row of the m x m inverse
__global__ void __launch_bounds__(BLOCK) k_dense_apply(int m, const double *__restrict__ inv, const int32_t *__restrict__ fr,
                                                       const double *__restrict__ b, double *x)
{
    __shared__ double sh[BLOCK];
    const int i = blockIdx.x;
    double acc = 0.0;
    for (int j = threadIdx.x; j < m; j += BLOCK) acc += inv[(long long)i * m + j] * b[fr[j]];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) x[fr[i]] = sh[0];
}

__global__ void k_mg_mask_copy(long long n, const uint8_t *freem, const double *x, double *y)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = freem[i] ? x[i] : 0.0;
}

__global__ void k_mg_add(long long n, const double *t, double *x)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] += t[i];
}

unsigned blocks_of(long long n) { return (unsigned)std::max<long long>(1, (n + BLOCK - 1) / BLOCK); }

} // namespace

namespace igx {

struct MgLevel {
    // the smoother
    int ncol = 0;
    std::vector<int> coff;                    // colour c: rows coff[c] .. coff[c + 1] of d_rows
    int32_t *d_rows = nullptr;                // free dofs sorted by (colour, index); a block solver: the nodes with a free component
    long long nnode = 0;                      // entries of d_rows (a scalar solver: nfree)
    int *d_coff = nullptr;
    bool one_block = false;
    int steps = 1;
    long long nfree = 0;                      // (a block solver: blocked free dofs)
    // the next coarser level, and the finer one that points here
    igx_solver *coarse = nullptr, *parent = nullptr;
    std::vector<Transfer> up, down;           // per patch: prolongation from / restriction to `coarse`
    int *d_bi = nullptr;                      // the bands' first columns and
    double *d_bv = nullptr;                   // weights
    double *d_winv = nullptr;                 // 1 / multiplicity of every dof of this level
    // the coarsest level
    double *d_inv = nullptr;
    int32_t *d_free = nullptr;
    int ninv = 0;
    // work vectors of this level: x | b | r | t, n each
    double *d_work = nullptr;
    long long n = 0;
    double *x() const { return d_work; }
    double *b() const { return d_work + n; }
    double *r() const { return d_work + 2 * n; }
    double *t() const { return d_work + 3 * n; }
};

} // namespace igx

namespace {

void drop_transfers(MgLevel *L)
{
    (void)hipFree(L->d_bi); (void)hipFree(L->d_bv); (void)hipFree(L->d_winv);
    L->d_bi = nullptr; L->d_bv = nullptr; L->d_winv = nullptr;
    L->up.clear(); L->down.clear();
}

// the level of a multipatch solver, made on first use with its work vectors
// (block: the call is one of igx_solver_set_block_mg_*, which serve the multipatch block solvers and no other)
int level_of(igx_solver *s, MgLevel **out, const char *what, bool block = false)
{
    const SolverRef R = solver_ref(s);
    if (!R.mp) { set_error("%s: multigrid needs a multipatch solver", what); return IGX_ERR_UNSUPPORTED; }
    if (R.ncomp > 1 && !block) {
        set_error("%s: a multipatch block solver (vector-valued system) takes its hierarchy through igx_solver_set_block_mg_*", what);
        return IGX_ERR_UNSUPPORTED;
    }
    if (R.ncomp < 2 && block) {
        set_error("%s: not a multipatch block solver (igx_solver_create_multipatch_block); a scalar one: igx_solver_set_mg_*", what);
        return IGX_ERR_UNSUPPORTED;
    }
    MgLevel *&L = solver_mg(s);
    if (!L) {
        IGX_HIP(hipSetDevice(R.ctx->device));
        double *w = nullptr;
        if (hipMalloc((void **)&w, 4 * (size_t)R.n * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: out of device memory (%.3f GB)", what, 4.0 * 8 * R.n / 1e9);
            return IGX_ERR_NOMEM;
        }
        IGX_HIP(hipMemsetAsync(w, 0, 4 * (size_t)R.n * sizeof(double), R.ctx->stream));
        IGX_HIP(hipStreamSynchronize(R.ctx->stream));
        L = new MgLevel;
        L->d_work = w;
        L->n = R.n;
        for (long long i = 0; i < R.n; ++i) L->nfree += R.h_free[i] ? 1 : 0;
    }
    *out = L;
    return IGX_OK;
}

// the solver `level` steps down the hierarchy from s (0: s itself)
igx_solver *walk(igx_solver *s, int level, const char *what)
{
    igx_solver *c = s;
    for (int l = 0; c && l <= level; ++l) {
        MgLevel *L = solver_mg(c);
        if (!L) break;
        if (l == level) return c;
        c = L->coarse;
    }
    set_error("%s: the hierarchy has no level %d", what, level);
    return nullptr;
}

// igx_solver_mg_profile_d: an event after every phase of a V-cycle (the time since the event before goes to the phase and level
// of the later one) and the number of kernel launches
enum { PH_START = 0, PH_SMOOTH, PH_RESIDUAL, PH_TRANSFER, PH_COARSE, PH_VECTOR };
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

// one sweep of the level's smoother on x, b (zero on the fixed dofs)
int sweep(hipStream_t st, igx_solver *s, MgLevel *L, double *x, const double *b, bool backward, Prof *pf = nullptr)
{
    const SolverRef R = solver_ref(s);
    const igx_multipatch *m = R.mp;
    if (R.ncomp > 1)
        return csr_node_gs_sweep(st, R.gw, R.ncomp, L->ncol, L->coff.data(), L->d_rows, R.N, m->d_indptr, m->d_indices, R.blk, R.d_mask,
                                 R.symmetric, x, b, backward, pf ? &pf->launches : nullptr);
    return csr_gs_sweep(st, R.gw, L->ncol, L->coff.data(), L->d_coff, L->d_rows, L->one_block, m->d_indptr, m->d_indices, m->d_vals, x, b,
                        backward, pf ? &pf->launches : nullptr);
}

// rc += P^T W^-1 rf (rf zero on the fixed dofs; rc cleared first).  A block solver: I (x) P^T, component after component on its
// slice of the vectors and of the mask (the transfers and the multiplicities are those of the scalar space)
int restrict_to(hipStream_t st, igx_solver *s, MgLevel *L, const double *rf, double *rc)
{
    const SolverRef F = solver_ref(s), C = solver_ref(L->coarse);
    IGX_HIP(hipMemsetAsync(rc, 0, (size_t)C.n * sizeof(double), st));
    for (int c = 0; c < C.ncomp; ++c)
        for (const Transfer &T : L->down) {
            k_mg_transfer<true><<<blocks_of(T.nout), BLOCK, 0, st>>>(T, C.d_mask + c * C.N, L->d_winv, rf + c * F.N, rc + c * C.N);
            IGX_HIP(hipGetLastError());
        }
    return IGX_OK;
}

// xf = P xc (xc zero on the fixed dofs)
int prolong_from(hipStream_t st, igx_solver *s, MgLevel *L, const double *xc, double *xf)
{
    const SolverRef F = solver_ref(s), C = solver_ref(L->coarse);
    IGX_HIP(hipMemsetAsync(xf, 0, (size_t)F.n * sizeof(double), st));
    for (int c = 0; c < F.ncomp; ++c)
        for (const Transfer &T : L->up) {
            k_mg_transfer<false><<<blocks_of(T.nout), BLOCK, 0, st>>>(T, F.d_mask + c * F.N, nullptr, xc + c * C.N, xf + c * F.N);
            IGX_HIP(hipGetLastError());
        }
    return IGX_OK;
}

int vcycle(hipStream_t st, igx_solver *s, const double *b, double *x, Prof *pf = nullptr, int lvl = 0)
{
    MgLevel *L = solver_mg(s);
    const SolverRef R = solver_ref(s);
    IGX_HIP(hipMemsetAsync(x, 0, (size_t)R.n * sizeof(double), st));
    if (L->d_inv) {
        if (int rc = dense_apply(st, L->ninv, L->d_inv, L->d_free, b, x)) return rc;
        if (pf) ++pf->launches;
        return mark(pf, lvl, PH_COARSE);
    }
    for (int k = 0; k < L->steps; ++k)
        if (int rc = sweep(st, s, L, x, b, false, pf)) return rc;
    if (int rc = mark(pf, lvl, PH_SMOOTH)) return rc;
    if (int rc = solver_residual(st, s, x, b, L->r())) return rc;
    if (int rc = mark(pf, lvl, PH_RESIDUAL)) return rc;
    MgLevel *LC = solver_mg(L->coarse);
    if (int rc = restrict_to(st, s, L, L->r(), LC->b())) return rc;
    if (int rc = mark(pf, lvl, PH_TRANSFER)) return rc;
    if (int rc = vcycle(st, L->coarse, LC->b(), LC->x(), pf, lvl + 1)) return rc;
    if (int rc = prolong_from(st, s, L, LC->x(), L->t())) return rc;
    if (int rc = mark(pf, lvl, PH_TRANSFER)) return rc;
    k_mg_add<<<blocks_of(R.n), BLOCK, 0, st>>>(R.n, L->t(), x);
    IGX_HIP(hipGetLastError());
    if (int rc = mark(pf, lvl, PH_VECTOR)) return rc;
    for (int k = 0; k < L->steps; ++k)
        if (int rc = sweep(st, s, L, x, b, true, pf)) return rc;
    if (pf) pf->launches += 2 + 2 * R.ncomp * (int)L->up.size();          // (the residual, the transfers of every patch and component, the sum)
    return mark(pf, lvl, PH_SMOOTH);
}

// the band of the rows of the nr x nc row-major matrix M (transposed: of its columns): first source index and w weights per row
void make_band(const double *M, int nr, int nc, bool transposed, std::vector<int> &lo, std::vector<double> &v, int &w)
{
    const int no = transposed ? nc : nr, ni = transposed ? nr : nc;
    auto at = [&](int o, int i) { return transposed ? M[(size_t)i * nc + o] : M[(size_t)o * nc + i]; };
    std::vector<int> first(no, 0), last(no, -1);
    w = 1;
    for (int o = 0; o < no; ++o) {
        int f = -1, l = -1;
        for (int i = 0; i < ni; ++i)
            if (at(o, i) != 0.0) { if (f < 0) f = i; l = i; }
        first[o] = f < 0 ? 0 : f;
        last[o] = l;
        if (f >= 0) w = std::max(w, l - f + 1);
    }
    lo.assign(no, 0);
    v.assign((size_t)no * w, 0.0);
    for (int o = 0; o < no; ++o) {
        lo[o] = std::max(0, std::min(first[o], ni - w));
        for (int t = 0; t < w && lo[o] + t < ni; ++t) v[(size_t)o * w + t] = at(o, lo[o] + t);
    }
}

} // namespace

namespace igx {

int csr_gs_sweep(hipStream_t st, int gw, int ncol, const int *coff, const int *d_coff, const int32_t *d_rows, bool one_block,
                 const int32_t *d_indptr, const int32_t *d_indices, const double *d_vals, double *x, const double *b, bool backward,
                 int *launches)
{
    if (one_block) {
        with_gs_kernel(gw, [&](auto, auto kb) {
            kb<<<1, BLOCK_ONE, 0, st>>>(ncol, d_coff, d_rows, d_indptr, d_indices, d_vals, x, b, backward ? 1 : 0);
        });
        if (launches) ++*launches;
    } else {
        const long long groups = BLOCK / gw;
        for (int ci = 0; ci < ncol; ++ci) {
            const int c = backward ? ncol - 1 - ci : ci;
            const long long nr = coff[c + 1] - coff[c];
            if (nr == 0) continue;
            const unsigned nb = (unsigned)std::min<long long>(NB_GS_MAX, (nr + groups - 1) / groups);
            with_gs_kernel(gw, [&](auto k, auto) {
                k<<<nb, BLOCK, 0, st>>>(nr, d_rows + coff[c], d_indptr, d_indices, d_vals, x, b);
            });
            if (launches) ++*launches;
        }
    }
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

int dense_apply(hipStream_t st, int m, const double *d_inv, const int32_t *d_idx, const double *b, double *x)
{
    if (m > 0) k_dense_apply<<<(unsigned)m, BLOCK, 0, st>>>(m, d_inv, d_idx, b, x);
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

void mg_free(igx_solver *s)
{
    MgLevel *&L = solver_mg(s);
    if (!L) return;
    if (L->parent) {                              // the finer level loses its coarse level, and with it the preconditioner
        MgLevel *P = solver_mg(L->parent);
        if (P) { P->coarse = nullptr; drop_transfers(P); }
        solver_drop_mg_precond(L->parent);
    }
    if (L->coarse && solver_mg(L->coarse)) solver_mg(L->coarse)->parent = nullptr;
    drop_transfers(L);
    (void)hipFree(L->d_rows); (void)hipFree(L->d_coff); (void)hipFree(L->d_inv); (void)hipFree(L->d_free); (void)hipFree(L->d_work);
    delete L;
    L = nullptr;
}

int mg_check(const igx_solver *s0, const char *what)
{
    igx_solver *s = const_cast<igx_solver *>(s0);
    for (int l = 0; ; ++l) {
        MgLevel *L = solver_mg(s);
        if (!L) { set_error("%s: multigrid level %d is not set up (igx_solver_set_mg_smoother / igx_solver_set_mg_inverse)", what, l); return IGX_ERR_ARG; }
        if (int rc = solver_check_sums(s, what)) return rc;
        if (L->d_inv) return IGX_OK;
        if (!L->d_rows) { set_error("%s: multigrid level %d has no smoother (igx_solver_set_mg_smoother)", what, l); return IGX_ERR_ARG; }
        if (!L->coarse) {
            set_error("%s: multigrid level %d has neither a coarser level (igx_solver_set_mg_coarse) nor an inverse "
                      "(igx_solver_set_mg_inverse)", what, l);
            return IGX_ERR_ARG;
        }
        s = L->coarse;
    }
}

int mg_apply(hipStream_t st, igx_solver *s, const double *r, double *z) { return vcycle(st, s, r, z); }

} // namespace igx

extern "C" {

int igx_csr_colouring(int64_t n, const int32_t *indptr, const int32_t *indices, const uint8_t *free_mask, int32_t *colour,
                      int32_t *ncolours)
{
    if (n < 0 || !indptr || (!indices && n > 0 && indptr[n] > 0) || !colour) { set_error("igx_csr_colouring: bad argument"); return IGX_ERR_ARG; }
    int32_t nc = 0;
    std::vector<int64_t> seen;                    // seen[c] == i: colour c is taken by a neighbour of row i
    for (int64_t i = 0; i < n; ++i) colour[i] = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (free_mask && !free_mask[i]) continue;
        for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k) {
            const int32_t j = indices[k];
            if (j < 0 || j >= n) { set_error("igx_csr_colouring: column %d of row %lld out of range", j, (long long)i); return IGX_ERR_ARG; }
            if (j != i && colour[j] >= 0) seen[colour[j]] = i;
        }
        int32_t c = 0;
        while (c < nc && seen[c] == i) ++c;
        if (c == nc) { ++nc; seen.push_back(-1); }
        colour[i] = c;
    }
    if (ncolours) *ncolours = nc;
    return IGX_OK;
}

} // extern "C"

namespace {

// igx_solver_set_mg_smoother, and igx_solver_set_block_mg_smoother (block): there the colours are those of the nodes, the scalar
// rows of the pattern, and a node is relaxed if any of its components is free
int set_smoother(igx_solver *s, const int32_t *colour, int smooth_steps, int64_t block_rows, bool block, const char *what)
{
    if (!s || !colour) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (smooth_steps < 1 || smooth_steps > 16) { set_error("%s: smooth_steps must be 1 .. 16, not %d", what, smooth_steps); return IGX_ERR_ARG; }
    MgLevel *L = nullptr;
    if (int rc = level_of(s, &L, what, block)) return rc;
    const SolverRef R = solver_ref(s);
    const igx_multipatch *m = R.mp;
    const char *dof = block ? "node" : "dof";
    auto is_free = [&](long long i) {
        for (int c = 0; c < R.ncomp; ++c)
            if (R.h_free[c * R.N + i]) return true;
        return false;
    };
    IGX_HIP(hipSetDevice(R.ctx->device));
    hipStream_t st = R.ctx->stream;
    // the pattern, to see that no row has a neighbour of its own colour
    std::vector<int32_t> ip((size_t)R.N + 1), ix((size_t)m->nnz);
    IGX_HIP(hipStreamSynchronize(st));
    IGX_HIP(hipMemcpy(ip.data(), m->d_indptr, ip.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (!ix.empty()) IGX_HIP(hipMemcpy(ix.data(), m->d_indices, ix.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    int ncol = 0;
    long long nnode = 0;
    for (long long i = 0; i < R.N; ++i) {
        if (!is_free(i)) continue;
        ++nnode;
        if (colour[i] < 0) { set_error("%s: free %s %lld has no colour", what, dof, i); return IGX_ERR_ARG; }
        ncol = std::max(ncol, colour[i] + 1);
        for (long long k = ip[i]; k < ip[i + 1]; ++k) {
            const int32_t j = ix[k];
            if (j != i && is_free(j) && colour[j] == colour[i]) {
                set_error("%s: %ss %lld and %d are coupled and both have colour %d", what, dof, i, j, colour[i]);
                return IGX_ERR_ARG;
            }
        }
    }
    std::vector<int> coff((size_t)ncol + 1, 0);
    for (long long i = 0; i < R.N; ++i)
        if (is_free(i)) ++coff[colour[i] + 1];
    for (int c = 0; c < ncol; ++c) coff[c + 1] += coff[c];
    std::vector<int32_t> rows((size_t)nnode);
    {
        std::vector<int> at(coff.begin(), coff.end() - 1);
        for (long long i = 0; i < R.N; ++i)
            if (is_free(i)) rows[at[colour[i]]++] = (int32_t)i;
    }
    (void)hipFree(L->d_rows); (void)hipFree(L->d_coff);
    L->d_rows = nullptr; L->d_coff = nullptr;
    IGX_HIP(hipMalloc((void **)&L->d_rows, std::max<size_t>(1, rows.size()) * sizeof(int32_t)));
    IGX_HIP(hipMalloc((void **)&L->d_coff, coff.size() * sizeof(int)));
    if (!rows.empty()) IGX_HIP(hipMemcpy(L->d_rows, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    IGX_HIP(hipMemcpy(L->d_coff, coff.data(), coff.size() * sizeof(int), hipMemcpyHostToDevice));
    L->ncol = ncol;
    L->coff = std::move(coff);
    L->nnode = nnode;
    L->steps = smooth_steps;
    L->one_block = !block && L->nfree <= block_rows;            // (the node sweep has no one-block variant)
    return IGX_OK;
}

// igx_solver_set_mg_coarse, and igx_solver_set_block_mg_coarse (block): P and mult are those of the scalar space
int set_coarse(igx_solver *s, igx_solver *coarse, const double *const *P, const double *mult, bool block, const char *what)
{
    if (!s || !coarse || !P || !mult || s == coarse) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    MgLevel *L = nullptr, *LC = nullptr;
    if (int rc = level_of(s, &L, what, block)) return rc;
    if (int rc = level_of(coarse, &LC, what, block)) return rc;
    const SolverRef F = solver_ref(s), Cc = solver_ref(coarse);
    const igx_multipatch *mf = F.mp, *mc = Cc.mp;
    if (F.ctx != Cc.ctx) { set_error("%s: the two solvers live on different contexts", what); return IGX_ERR_ARG; }
    if (F.ncomp != Cc.ncomp) { set_error("%s: %d fine and %d coarse components", what, F.ncomp, Cc.ncomp); return IGX_ERR_ARG; }
    if (!mf->injective || !mc->injective) {
        set_error("%s: a local-to-global map is not injective (two dofs of one patch share a global dof): the transfers need "
                  "injective maps", what);
        return IGX_ERR_UNSUPPORTED;
    }
    if (mf->np != mc->np) { set_error("%s: %d fine and %d coarse patches", what, mf->np, mc->np); return IGX_ERR_ARG; }
    if (LC->parent && LC->parent != s) { set_error("%s: the coarse solver is the next level of another solver already", what); return IGX_ERR_ARG; }
    for (igx_solver *c = coarse; c; c = solver_mg(c) ? solver_mg(c)->coarse : nullptr)
        if (c == s) { set_error("%s: the hierarchy would contain a cycle", what); return IGX_ERR_ARG; }
    for (long long i = 0; i < F.N; ++i)
        if (!(mult[i] >= 1.0)) { set_error("%s: multiplicity %g of dof %lld", what, mult[i], i); return IGX_ERR_ARG; }
    // the bands of every patch and axis: [P rows | P columns], 2D patches get a one-dof outer axis
    std::vector<int> bi;
    std::vector<double> bv;
    struct Pos { size_t lo, v; int w; };
    std::vector<Pos> pos;                          // per patch: 3 axes up, then 3 axes down
    for (int p = 0; p < mf->np; ++p) {
        const auto &A = mf->pp[p], &B = mc->pp[p];
        if (A.dim != B.dim) { set_error("%s: patch %d has dimension %d and %d", what, p, A.dim, B.dim); return IGX_ERR_ARG; }
        const int off = 3 - A.dim;
        for (int dir = 0; dir < 2; ++dir)
            for (int a = 0; a < 3; ++a) {
                std::vector<int> lo;
                std::vector<double> v;
                int w = 1;
                if (a < off) { lo = {0}; v = {1.0}; }
                else {
                    const double *M = P[p * 3 + a - off];
                    if (!M) { set_error("%s: patch %d: prolongation of axis %d missing", what, p, a - off); return IGX_ERR_ARG; }
                    make_band(M, A.N[a - off], B.N[a - off], dir == 1, lo, v, w);
                }
                pos.push_back(Pos{bi.size(), bv.size(), w});
                bi.insert(bi.end(), lo.begin(), lo.end());
                bv.insert(bv.end(), v.begin(), v.end());
            }
    }
    std::vector<double> winv((size_t)F.N);
    for (long long i = 0; i < F.N; ++i) winv[i] = 1.0 / mult[i];
    IGX_HIP(hipSetDevice(F.ctx->device));
    IGX_HIP(hipStreamSynchronize(F.ctx->stream));
    if (L->coarse && L->coarse != coarse && solver_mg(L->coarse)) solver_mg(L->coarse)->parent = nullptr;
    L->coarse = nullptr;
    drop_transfers(L);
    solver_drop_mg_precond(s);
    IGX_HIP(hipMalloc((void **)&L->d_bi, bi.size() * sizeof(int)));
    IGX_HIP(hipMalloc((void **)&L->d_bv, bv.size() * sizeof(double)));
    IGX_HIP(hipMalloc((void **)&L->d_winv, winv.size() * sizeof(double)));
    IGX_HIP(hipMemcpy(L->d_bi, bi.data(), bi.size() * sizeof(int), hipMemcpyHostToDevice));
    IGX_HIP(hipMemcpy(L->d_bv, bv.data(), bv.size() * sizeof(double), hipMemcpyHostToDevice));
    IGX_HIP(hipMemcpy(L->d_winv, winv.data(), winv.size() * sizeof(double), hipMemcpyHostToDevice));
    for (int p = 0; p < mf->np; ++p) {
        const auto &A = mf->pp[p], &B = mc->pp[p];
        const int off = 3 - A.dim;
        Transfer U{}, D{};
        for (int a = 0; a < 3; ++a) {
            const int nf = a < off ? 1 : A.N[a - off], nc = a < off ? 1 : B.N[a - off];
            const Pos &u = pos[(size_t)p * 6 + a], &d = pos[(size_t)p * 6 + 3 + a];
            U.No[a] = nf; U.Ni[a] = nc; U.w[a] = u.w; U.lo[a] = L->d_bi + u.lo; U.v[a] = L->d_bv + u.v;
            D.No[a] = nc; D.Ni[a] = nf; D.w[a] = d.w; D.lo[a] = L->d_bi + d.lo; D.v[a] = L->d_bv + d.v;
        }
        U.l2g_o = A.d_l2g; U.l2g_i = B.d_l2g; U.nout = A.n;
        D.l2g_o = B.d_l2g; D.l2g_i = A.d_l2g; D.nout = B.n;
        L->up.push_back(U);
        L->down.push_back(D);
    }
    L->coarse = coarse;
    LC->parent = s;
    return IGX_OK;
}

// igx_solver_set_mg_inverse, and igx_solver_set_block_mg_inverse (block): there the free dofs are blocked, ascending
int set_inverse(igx_solver *s, const double *inv, int64_t m, bool block, const char *what)
{
    if (!s || (!inv && m > 0)) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    MgLevel *L = nullptr;
    if (int rc = level_of(s, &L, what, block)) return rc;
    if (m != L->nfree) { set_error("%s: the inverse has %lld rows, the level %lld free dofs", what, (long long)m, L->nfree); return IGX_ERR_ARG; }
    if (m > 8192) { set_error("%s: %lld free dofs are too many for a dense inverse", what, (long long)m); return IGX_ERR_UNSUPPORTED; }
    const SolverRef R = solver_ref(s);
    std::vector<int32_t> fr;
    for (long long i = 0; i < R.n; ++i)
        if (R.h_free[i]) fr.push_back((int32_t)i);
    IGX_HIP(hipSetDevice(R.ctx->device));
    IGX_HIP(hipStreamSynchronize(R.ctx->stream));
    (void)hipFree(L->d_inv); (void)hipFree(L->d_free);
    L->d_inv = nullptr; L->d_free = nullptr;
    IGX_HIP(hipMalloc((void **)&L->d_inv, std::max<size_t>(1, (size_t)m * m) * sizeof(double)));
    IGX_HIP(hipMalloc((void **)&L->d_free, std::max<size_t>(1, (size_t)m) * sizeof(int32_t)));
    if (m > 0) {
        IGX_HIP(hipMemcpy(L->d_inv, inv, (size_t)m * m * sizeof(double), hipMemcpyHostToDevice));
        IGX_HIP(hipMemcpy(L->d_free, fr.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    L->ninv = (int)m;
    return IGX_OK;
}

} // namespace

extern "C" {

int igx_solver_set_mg_smoother(igx_solver *s, const int32_t *colour, int smooth_steps, int64_t block_rows)
{
    return set_smoother(s, colour, smooth_steps, block_rows, false, "igx_solver_set_mg_smoother");
}

int igx_solver_set_mg_coarse(igx_solver *s, igx_solver *coarse, const double *const *P, const double *mult)
{
    return set_coarse(s, coarse, P, mult, false, "igx_solver_set_mg_coarse");
}

int igx_solver_set_mg_inverse(igx_solver *s, const double *inv, int64_t m)
{
    return set_inverse(s, inv, m, false, "igx_solver_set_mg_inverse");
}

int igx_solver_set_block_mg_smoother(igx_solver *s, const int32_t *colour, int smooth_steps)
{
    return set_smoother(s, colour, smooth_steps, 0, true, "igx_solver_set_block_mg_smoother");
}

int igx_solver_set_block_mg_coarse(igx_solver *s, igx_solver *coarse, const double *const *P, const double *mult)
{
    return set_coarse(s, coarse, P, mult, true, "igx_solver_set_block_mg_coarse");
}

int igx_solver_set_block_mg_inverse(igx_solver *s, const double *inv, int64_t m)
{
    return set_inverse(s, inv, m, true, "igx_solver_set_block_mg_inverse");
}

int igx_solver_mg_info(igx_solver *s, int level, igx_mg_info *out)
{
    const char *what = "igx_solver_mg_info";
    if (!s || !out || level < 0) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    igx_solver *c = walk(s, level, what);
    if (!c) return IGX_ERR_ARG;
    const MgLevel *L = solver_mg(c);
    const SolverRef R = solver_ref(c);
    std::memset(out, 0, sizeof(*out));
    out->nrows = R.n;
    out->nfree = L->nfree;
    out->nnz = R.mp->nnz;
    if (R.ncomp > 1) {                            // (the present blocks, each over the whole pattern)
        int present = 0;
        for (int k = 0; k < R.ncomp * R.ncomp; ++k) present += R.blk[k] ? 1 : 0;
        out->nnz *= present;
    }
    out->ncolours = L->ncol;
    out->one_block = L->one_block ? 1 : 0;
    out->smooth_steps = L->steps;
    out->dense_inverse = L->d_inv ? 1 : 0;
    out->has_coarse = L->coarse ? 1 : 0;
    return IGX_OK;
}

int igx_solver_mg_colours(igx_solver *s, int level, int32_t *rows, int32_t *colour_offsets)
{
    const char *what = "igx_solver_mg_colours";
    if (!s || !rows || !colour_offsets || level < 0) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    igx_solver *c = walk(s, level, what);
    if (!c) return IGX_ERR_ARG;
    const MgLevel *L = solver_mg(c);
    if (!L->d_rows) { set_error("%s: level %d has no smoother", what, level); return IGX_ERR_ARG; }
    const SolverRef R = solver_ref(c);
    IGX_HIP(hipSetDevice(R.ctx->device));
    IGX_HIP(hipStreamSynchronize(R.ctx->stream));
    if (L->nnode > 0) IGX_HIP(hipMemcpy(rows, L->d_rows, (size_t)L->nnode * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int k = 0; k <= L->ncol; ++k) colour_offsets[k] = L->coff[k];
    return IGX_OK;
}

int igx_solver_mg_profile_d(igx_solver *s, const double *d_r, double *d_z, int reps, igx_mg_profile *out)
{
    const char *what = "igx_solver_mg_profile_d";
    if (!s || !d_r || !d_z || d_r == d_z || !out || reps < 1) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    if (int rc = mg_check(s, what)) return rc;
    MgLevel *L = solver_mg(s);
    const SolverRef R = solver_ref(s);
    IGX_HIP(hipSetDevice(R.ctx->device));
    hipStream_t st = R.ctx->stream;
    std::memset(out, 0, sizeof(*out));
    k_mg_mask_copy<<<blocks_of(R.n), BLOCK, 0, st>>>(R.n, R.d_mask, d_r, L->b());
    IGX_HIP(hipGetLastError());
    for (int rep = 0; rep < reps; ++rep) {
        Prof pf;
        pf.st = st;
        int rc = mark(&pf, 0, PH_START);
        if (!rc) rc = vcycle(st, s, L->b(), d_z, &pf, 0);
        const hipError_t e = hipStreamSynchronize(st);
        if (!rc && e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); rc = IGX_ERR_HIP; }
        for (size_t k = 1; !rc && k < pf.ev.size(); ++k) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, pf.ev[k - 1], pf.ev[k]);
            const int l = std::min(pf.level[k], IGX_MG_MAX_LEVELS - 1);
            out->total_ms += ms;
            switch (pf.phase[k]) {
            case PH_SMOOTH: out->smooth_ms[l] += ms; break;
            case PH_RESIDUAL: out->residual_ms[l] += ms; break;
            case PH_TRANSFER: out->transfer_ms[l] += ms; break;
            case PH_COARSE: out->coarse_ms += ms; out->levels = pf.level[k] + 1; break;
            default: out->vector_ms += ms; break;
            }
        }
        for (hipEvent_t ev : pf.ev) (void)hipEventDestroy(ev);
        if (rc) return rc;
        out->launches = pf.launches;
    }
    const float inv = 1.0f / (float)reps;
    out->total_ms *= inv; out->coarse_ms *= inv; out->vector_ms *= inv;
    for (int l = 0; l < IGX_MG_MAX_LEVELS; ++l) { out->smooth_ms[l] *= inv; out->residual_ms[l] *= inv; out->transfer_ms[l] *= inv; }
    return IGX_OK;
}

int igx_solver_mg_relax_d(igx_solver *s, int level, int backward, const double *d_b, double *d_x)
{
    const char *what = "igx_solver_mg_relax_d";
    if (!s || !d_b || !d_x || level < 0) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    igx_solver *c = walk(s, level, what);
    if (!c) return IGX_ERR_ARG;
    MgLevel *L = solver_mg(c);
    if (!L->d_rows) { set_error("%s: level %d has no smoother (igx_solver_set_mg_smoother)", what, level); return IGX_ERR_ARG; }
    if (int rc = solver_check_sums(c, what)) return rc;
    const SolverRef R = solver_ref(c);
    IGX_HIP(hipSetDevice(R.ctx->device));
    hipStream_t st = R.ctx->stream;
    k_mg_mask_copy<<<blocks_of(R.n), BLOCK, 0, st>>>(R.n, R.d_mask, d_x, L->x());
    k_mg_mask_copy<<<blocks_of(R.n), BLOCK, 0, st>>>(R.n, R.d_mask, d_b, L->b());
    IGX_HIP(hipGetLastError());
    if (int rc = sweep(st, c, L, L->x(), L->b(), backward != 0)) return rc;
    IGX_HIP(hipMemcpyAsync(d_x, L->x(), (size_t)R.n * sizeof(double), hipMemcpyDeviceToDevice, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_solver_mg_prolong_d(igx_solver *s, int level, const double *d_xc, double *d_xf)
{
    const char *what = "igx_solver_mg_prolong_d";
    if (!s || !d_xc || !d_xf || level < 0) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    igx_solver *f = walk(s, level, what);
    if (!f) return IGX_ERR_ARG;
    MgLevel *L = solver_mg(f);
    if (!L->coarse) { set_error("%s: level %d has no coarser level (igx_solver_set_mg_coarse)", what, level); return IGX_ERR_ARG; }
    MgLevel *LC = solver_mg(L->coarse);
    const SolverRef R = solver_ref(f), Cc = solver_ref(L->coarse);
    IGX_HIP(hipSetDevice(R.ctx->device));
    hipStream_t st = R.ctx->stream;
    k_mg_mask_copy<<<blocks_of(Cc.n), BLOCK, 0, st>>>(Cc.n, Cc.d_mask, d_xc, LC->x());
    IGX_HIP(hipGetLastError());
    if (int rc = prolong_from(st, f, L, LC->x(), d_xf)) return rc;
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_solver_mg_restrict_d(igx_solver *s, int level, const double *d_rf, double *d_rc)
{
    const char *what = "igx_solver_mg_restrict_d";
    if (!s || !d_rf || !d_rc || level < 0) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    igx_solver *f = walk(s, level, what);
    if (!f) return IGX_ERR_ARG;
    MgLevel *L = solver_mg(f);
    if (!L->coarse) { set_error("%s: level %d has no coarser level (igx_solver_set_mg_coarse)", what, level); return IGX_ERR_ARG; }
    const SolverRef R = solver_ref(f);
    IGX_HIP(hipSetDevice(R.ctx->device));
    hipStream_t st = R.ctx->stream;
    k_mg_mask_copy<<<blocks_of(R.n), BLOCK, 0, st>>>(R.n, R.d_mask, d_rf, L->r());
    IGX_HIP(hipGetLastError());
    if (int rc = restrict_to(st, f, L, L->r(), d_rc)) return rc;
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

} // extern "C"
