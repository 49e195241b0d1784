// Dirichlet problems solved on the device: preconditioned CG on the values igx_assemble left in HBM (one patch), or on the
// global sums igx_multipatch_* formed there (several patches) (igx_solver_*, igx_kron_apply_d; include/igx.h).
//
// Replaces the host steps of the reference's workflow  RestrictedLinearSystem -> make_solver / cg  (pyiga/assemble.py:571-652,
// pyiga/solvers.py:17-42, pyiga/approx.py:62-96) for a single patch.  Three kinds of kernels:
//   k_spmv     y = R A R^T x  (and  b - A ext(g)): reads the CSR values in the patch's structured layout
//              -- positions from the per-axis tables rp / jlo / jhi, no indices / indptr: 8 bytes per nonzero.  One group of GW
//              lanes per row; rows of fixed dofs are not read and come out as 0.
//   k_kron     one contraction  Y[.., i, ..] = sum_j B[i][j] X[.., j, ..]  of a Kronecker product through LDS tiles (FP64 VALU);
//              strided input / output, so the fast-diagonalization preconditioner (Sangalli-Tani) works on the free box of a
//              full-length vector.  The last contraction can divide by the eigenvalue sums / products (D^-1).
//   k_csr_spmv the same product over the general CSR pattern of a multipatch (indptr / indices / values: 12 bytes per
//              nonzero), k_csr_diag its diagonal; the additive Schwarz preconditioner gathers the box of every patch
//              (k_box_gather), applies the patch's fast-diagonalization inverse with the k_kron steps and adds it back
//              (k_box_scatter), patch after patch.
//   k_block_spmv  the product of a vector-valued form's NC x NC blocks (NC = 2, 3), which share the patch's layout: one group per
//              scalar row computes the NC outputs (igx_solver_create_block).
//   k_csr_block_spmv  the same product for the blocks of a vector-valued form on a multipatch, which share its global CSR
//              pattern (igx_solver_create_multipatch_block); Schwarz then acts component by component.
//   vector     fused CG updates and fixed-order two-pass dot products (fixed grid, fixed trees): two solves of the same
//              system give bit-identical results.  alpha and beta stay in device memory.
//   BiCGStab   for non-symmetric matrices (igx_solver_create_general / igx_solver_set_method): the same SpMVs and
//              preconditioners, fused p / s / x-r updates that emit their dot partials, and k_fin_bicg for rho, alpha, omega,
//              the stop and breakdown on the device.
// Host side: one dispatch table per SpMV family (with_spmv_kernel, with_csr_spmv_kernel, ...) names the instantiations, for the launch
// and the occupancy query alike; one fast-diagonalization block (FastDiag) is the Kronecker preconditioner of a patch and the
// local solve of every Schwarz patch; igx_solver_solve forms the lifted right-hand side and hands over to solve_cg or
// solve_bicgstab.  Newton's method on a patch solver is the same solve for the increment.
// The time stepping of parabolic problems is in solve_step.hip, the block eigen-solver in solve_eig.hip and the saddle-point solver
// (MINRES; its entry points here hand over where s->saddle is set) in solve_saddle.hip; solve_internal.h holds the solver structure
// and what the units call of each other.
#include "solve_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace igx;

namespace {

enum { SC_PQ = 0, SC_RZ, SC_RR, SC_ALPHA, SC_BETA, SC_N = 8 };
enum { FIN_ALPHA = 0, FIN_BETA = 1, FIN_INIT = 2 };

// y[I] = free[I] ? (b ? b[I] : 0) + s * (A x)[I] : 0 ;  part[block] = sum of pd[I] * y[I] over the rows of the block (optional)
// (U batches of GW values per lane are loaded before they are summed: enough bytes in flight to stream HBM; the values are read
// once, non-temporally, so that x stays in the caches)
template <int GW, int U>
__global__ void __launch_bounds__(BLOCK) k_spmv(const Geom g, const double *__restrict__ vals, const uint8_t *__restrict__ freem,
                                                const double *__restrict__ x, const double *b, double s, double *y,
                                                const double *__restrict__ pd, double *part)
{
    __shared__ double sh[BLOCK];
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    const int N1 = g.N[1], N2 = g.N[2];
    const int N12 = N1 * N2;
    double dot = 0.0;
    long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW;
    RowHdr h{};
    if (I < g.nrows) h = row_hdr(g, freem, I);
    for (; I < g.nrows; I += ngroups) {
        const RowHdr cur = h;
        if (I + ngroups < g.nrows) h = row_hdr(g, freem, I + ngroups);
        if (!cur.fr) {                               // (uniform over the group)
            if (lane == 0) y[I] = 0.0;
            continue;
        }
        const int c0 = cur.c0 - cur.l0, c1 = cur.c1 - cur.l1, c2 = cur.c2 - cur.l2;
        const int len = c0 * c1 * c2;
        const long long row = igx_rowptr3(&cur.r0, &cur.r1, &cur.r2, g.S1, g.S2, c0, c1, 0, 0, 0);
        const int xbase = (cur.l0 * N1 + cur.l1) * N2 + cur.l2;
        // lane's entry k = (a c1 + bb) c2 + c, advanced by GW = (da c1 + db) c2 + dc per step
        int c = lane % c2, bb = (lane / c2) % c1, a = lane / (c1 * c2);
        const int dc = GW % c2, db = (GW / c2) % c1, da = GW / (c1 * c2);
        double acc = 0.0;
        for (int k0 = lane; k0 < len; k0 += U * GW) {
            double v[U], xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k0 + u * GW < len;
                v[u] = in ? __builtin_nontemporal_load(vals + row + k0 + u * GW) : 0.0;
                xv[u] = in ? x[xbase + a * N12 + bb * N2 + c] : 0.0;
                c += dc; bb += db; a += da;
                if (c >= c2) { c -= c2; ++bb; }
                if (bb >= c1) { bb -= c1; ++a; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) acc += v[u] * xv[u];
        }
#pragma unroll
        for (int off = GW / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, GW);
        if (lane == 0) {
            const double v = (b ? b[I] : 0.0) + s * acc;
            y[I] = v;
            if (pd) dot += pd[I] * v;
        }
    }
    if (part) {
        const double v = block_sum(dot, sh);
        if (threadIdx.x == 0) part[blockIdx.x] = v;
    }
}

// The contract of k_spmv over the block matrix [A_pq].  Vectors have NC * N entries, component-major
// (x_q[J] = x[q N + J]): y[p N + I] = free[p N + I] ? (b ? b[p N + I] : 0) + s * sum_q (A_pq x_q)[I] : 0, part[block] = sum of
// pd . y over the NC outputs of the rows of the block (optional).  All blocks share the patch's pattern: one group of GW lanes per
// scalar row I decodes the row header and the lane's position once per entry, gathers x_q[J] once for all NC outputs and streams
// the NC^2 values of the entry.  Absent blocks (uniform over the grid) and the rows of fixed components (uniform over the group)
// are not read.
template <int GW, int U, int NC>
__global__ void __launch_bounds__(BLOCK) k_block_spmv(const Geom g, const BlockVals A, const uint8_t *__restrict__ freem,
                                                      const double *__restrict__ x, const double *b, double s, double *y,
                                                      const double *__restrict__ pd, double *part)
{
    __shared__ double sh[BLOCK];
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    const long long N = g.nrows;
    const int N1 = g.N[1], N2 = g.N[2];
    const int N12 = N1 * N2;
    double dot = 0.0;
    long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW;
    RowHdr h{};
    if (I < N) h = row_hdr(g, freem, I);
    for (; I < N; I += ngroups) {
        const RowHdr cur = h;
        if (I + ngroups < N) h = row_hdr(g, freem, I + ngroups);
        bool fr[NC], any = false;
#pragma unroll
        for (int p = 0; p < NC; ++p) {
            fr[p] = freem[p * N + I] != 0;
            any = any || fr[p];
        }
        if (!any) {                                  // (uniform over the group)
            if (lane < NC) y[lane * N + I] = 0.0;
            continue;
        }
        const int c0 = cur.c0 - cur.l0, c1 = cur.c1 - cur.l1, c2 = cur.c2 - cur.l2;
        const int len = c0 * c1 * c2;
        const long long row = igx_rowptr3(&cur.r0, &cur.r1, &cur.r2, g.S1, g.S2, c0, c1, 0, 0, 0);
        const int xbase = (cur.l0 * N1 + cur.l1) * N2 + cur.l2;
        int c = lane % c2, bb = (lane / c2) % c1, a = lane / (c1 * c2);
        const int dc = GW % c2, db = (GW / c2) % c1, da = GW / (c1 * c2);
        double acc[NC];
#pragma unroll
        for (int p = 0; p < NC; ++p) acc[p] = 0.0;
        for (int k0 = lane; k0 < len; k0 += U * GW) {
            double v[U][NC][NC], xv[U][NC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k0 + u * GW < len;
                const long long J = xbase + a * N12 + bb * N2 + c;
#pragma unroll
                for (int q = 0; q < NC; ++q) xv[u][q] = in ? x[q * N + J] : 0.0;
#pragma unroll
                for (int p = 0; p < NC; ++p)
#pragma unroll
                    for (int q = 0; q < NC; ++q) {
                        const double *vp = A.v[p * NC + q];
                        v[u][p][q] = (in && fr[p] && vp) ? __builtin_nontemporal_load(vp + row + k0 + u * GW) : 0.0;
                    }
                c += dc; bb += db; a += da;
                if (c >= c2) { c -= c2; ++bb; }
                if (bb >= c1) { bb -= c1; ++a; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < NC; ++p)
#pragma unroll
                    for (int q = 0; q < NC; ++q) acc[p] += v[u][p][q] * xv[u][q];
        }
#pragma unroll
        for (int p = 0; p < NC; ++p)
#pragma unroll
            for (int off = GW / 2; off > 0; off >>= 1) acc[p] += __shfl_xor(acc[p], off, GW);
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < NC; ++p) {
                const long long o = p * N + I;
                const double v = fr[p] ? (b ? b[o] : 0.0) + s * acc[p] : 0.0;
                y[o] = v;
                if (pd) dot += pd[o] * v;
            }
        }
    }
    if (part) {
        const double v = block_sum(dot, sh);
        if (threadIdx.x == 0) part[blockIdx.x] = v;
    }
}

// dinv[I] = free[I] ? 1 / A[I][I] : 0  (the diagonal gathered from the structured layout)
__global__ void k_diag(const Geom g, const double *__restrict__ vals, const uint8_t *__restrict__ freem, double *dinv)
{
    const long long I = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= g.nrows) return;
    if (!freem[I]) { dinv[I] = 0.0; return; }
    const int N1 = g.N[1], N2 = g.N[2];
    const int i2 = (int)(I % N2);
    const long long t = I / N2;
    const int i1 = (int)(t % N1), i0 = (int)(t / N1);
    const int l0 = g.jlo[0][i0], l1 = g.jlo[1][i1], l2 = g.jlo[2][i2];
    const int c0 = g.jhi[0][i0] - l0, c1 = g.jhi[1][i1] - l1, c2 = g.jhi[2][i2] - l2;
    const long long row = igx_rowptr3(g.rp[0], g.rp[1], g.rp[2], g.S1, g.S2, c0, c1, i0, i1, i2);
    dinv[I] = 1.0 / vals[row + ((long long)(i0 - l0) * c1 + (i1 - l1)) * c2 + (i2 - l2)];
}

// the contract of k_spmv over the general CSR pattern of a multipatch: y[I] = free[I] ? (b ? b[I] : 0) + s * (A x)[I] : 0,
// part[block] = sum of pd[I] * y[I] over the rows of the block (optional).  Values and indices are streamed once
// (non-temporal), x is gathered through the caches.  Offsets into values / indices are 64-bit.
template <int GW, int U>
__global__ void __launch_bounds__(BLOCK) k_csr_spmv(long long nrows, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const double *__restrict__ vals, const uint8_t *__restrict__ freem,
                                                    const double *__restrict__ x, const double *b, double s, double *y,
                                                    const double *__restrict__ pd, double *part)
{
    __shared__ double sh[BLOCK];
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    double dot = 0.0;
    long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW;
    // row header loaded one row ahead
    long long nk0 = 0, nk1 = 0;
    int nfr = 0;
    if (I < nrows) { nfr = freem[I]; nk0 = indptr[I]; nk1 = indptr[I + 1]; }
    for (; I < nrows; I += ngroups) {
        const long long k0 = nk0, k1 = nk1;
        const int fr = nfr;
        if (I + ngroups < nrows) { nfr = freem[I + ngroups]; nk0 = indptr[I + ngroups]; nk1 = indptr[I + ngroups + 1]; }
        if (!fr) {                                   // (uniform over the group)
            if (lane == 0) y[I] = 0.0;
            continue;
        }
        double acc = 0.0;
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
            for (int u = 0; u < U; ++u) xv[u] = c[u] >= 0 ? x[c[u]] : 0.0;
#pragma unroll
            for (int u = 0; u < U; ++u) acc += v[u] * xv[u];
        }
#pragma unroll
        for (int off = GW / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, GW);
        if (lane == 0) {
            const double v = (b ? b[I] : 0.0) + s * acc;
            y[I] = v;
            if (pd) dot += pd[I] * v;
        }
    }
    if (part) {
        const double v = block_sum(dot, sh);
        if (threadIdx.x == 0) part[blockIdx.x] = v;
    }
}

// The contracts of k_csr_spmv and k_block_spmv together: the block matrix [A_pq] of a vector-valued form over the global CSR
// pattern of a multipatch, which all NC x NC blocks share.  Vectors have NC * N entries, component-major
// (x_q[J] = x[q N + J], N the scalar global dofs): y[p N + I] = free[p N + I] ? (b ? b[p N + I] : 0) + s * sum_q (A_pq x_q)[I] : 0,
// part[block] = sum of pd . y over the NC outputs of the rows of the block (optional).  One group of GW lanes per scalar global
// row I: per entry a lane loads the column index once, gathers x_q[J] for the NC trial components and streams the values of the
// blocks that are present (uniform over the grid) and whose test component is free in this row (uniform over the group).  Values
// and indices are read once, non-temporally, at 64-bit offsets; the row header (indptr and the NC free flags, bit p of fr) is
// loaded one row ahead.
template <int GW, int U, int NC>
__global__ void __launch_bounds__(BLOCK) k_csr_block_spmv(long long N, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                          const BlockVals A, const uint8_t *__restrict__ freem,
                                                          const double *__restrict__ x, const double *b, double s, double *y,
                                                          const double *__restrict__ pd, double *part)
{
    __shared__ double sh[BLOCK];
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    double dot = 0.0;
    long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW;
    auto row_flags = [&](long long R) {
        int f = 0;
#pragma unroll
        for (int p = 0; p < NC; ++p) f |= (freem[p * N + R] != 0) << p;
        return f;
    };
    long long nk0 = 0, nk1 = 0;
    int nfr = 0;
    if (I < N) { nfr = row_flags(I); nk0 = indptr[I]; nk1 = indptr[I + 1]; }
    for (; I < N; I += ngroups) {
        const long long k0 = nk0, k1 = nk1;
        const int fr = nfr;
        if (I + ngroups < N) { nfr = row_flags(I + ngroups); nk0 = indptr[I + ngroups]; nk1 = indptr[I + ngroups + 1]; }
        if (!fr) {                                   // (uniform over the group)
            if (lane < NC) y[lane * N + I] = 0.0;
            continue;
        }
        double acc[NC];
#pragma unroll
        for (int p = 0; p < NC; ++p) acc[p] = 0.0;
        for (long long k = k0 + lane; k < k1; k += U * GW) {
            double v[U][NC][NC], xv[U][NC];
            int c[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k + u * GW < k1;
                c[u] = in ? __builtin_nontemporal_load(indices + k + u * GW) : -1;
#pragma unroll
                for (int p = 0; p < NC; ++p)
#pragma unroll
                    for (int q = 0; q < NC; ++q) {
                        const double *vp = A.v[p * NC + q];
                        v[u][p][q] = (in && ((fr >> p) & 1) && vp) ? __builtin_nontemporal_load(vp + k + u * GW) : 0.0;
                    }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < NC; ++q) xv[u][q] = c[u] >= 0 ? x[q * N + c[u]] : 0.0;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < NC; ++p)
#pragma unroll
                    for (int q = 0; q < NC; ++q) acc[p] += v[u][p][q] * xv[u][q];
        }
#pragma unroll
        for (int p = 0; p < NC; ++p)
#pragma unroll
            for (int off = GW / 2; off > 0; off >>= 1) acc[p] += __shfl_xor(acc[p], off, GW);
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < NC; ++p) {
                const long long o = p * N + I;
                const double v = ((fr >> p) & 1) ? (b ? b[o] : 0.0) + s * acc[p] : 0.0;
                y[o] = v;
                if (pd) dot += pd[o] * v;
            }
        }
    }
    if (part) {
        const double v = block_sum(dot, sh);
        if (threadIdx.x == 0) part[blockIdx.x] = v;
    }
}

// dinv[I] = free[I] ? 1 / A[I][I] : 0, the diagonal found by binary search in the sorted row
__global__ void k_csr_diag(long long nrows, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                           const double *__restrict__ vals, const uint8_t *__restrict__ freem, double *dinv)
{
    const long long I = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nrows) return;
    if (!freem[I]) { dinv[I] = 0.0; return; }
    const long long end = indptr[I + 1];
    long long lo = indptr[I], hi = end;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (indices[mid] < I) lo = mid + 1; else hi = mid;
    }
    dinv[I] = (lo < end && indices[lo] == I) ? 1.0 / vals[lo] : 0.0;
}

__device__ __forceinline__ int box_global(const BoxMap &m, long long i)
{
    const int c2 = (int)(i % m.nb[2]);
    const long long t = i / m.nb[2];
    const int c1 = (int)(t % m.nb[1]), c0 = (int)(t / m.nb[1]);
    return m.l2g[((long long)(m.lo[0] + c0) * m.N[1] + (m.lo[1] + c1)) * m.N[2] + (m.lo[2] + c2)];
}

// rp[i] = free[g] ? r[g] : 0, g the global dof of box entry i
__global__ void k_box_gather(const BoxMap m, const uint8_t *__restrict__ freem, const double *__restrict__ r, double *__restrict__ rp)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m.nbox) return;
    const int g = box_global(m, i);
    rp[i] = freem[g] ? r[g] : 0.0;
}

// z[g] += zp[i] on the free g (the map of a patch is injective: no two entries of one pass meet)
__global__ void k_box_scatter(const BoxMap m, const uint8_t *__restrict__ freem, const double *__restrict__ zp, double *z)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m.nbox) return;
    const int g = box_global(m, i);
    if (freem[g]) z[g] += zp[i];
}

__global__ void k_scale(long long n, const double *d, const double *x, double *y)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = d[i] * x[i];
}

__global__ void k_mask_copy(long long n, const uint8_t *freem, const double *x, double *y)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = freem[i] ? x[i] : 0.0;
}

// partA[block] = sum a1 b1, partB[block] = sum a2 b2 (a2 may be null)
__global__ void __launch_bounds__(BLOCK) k_dot2(long long n, const double *a1, const double *b1, const double *a2, const double *b2,
                                                double *partA, double *partB)
{
    __shared__ double sh[BLOCK];
    double s1 = 0.0, s2 = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        s1 += a1[i] * b1[i];
        if (a2) s2 += a2[i] * b2[i];
    }
    s1 = block_sum(s1, sh);
    if (threadIdx.x == 0) partA[blockIdx.x] = s1;
    if (a2) {
        s2 = block_sum(s2, sh);
        if (threadIdx.x == 0) partB[blockIdx.x] = s2;
    }
}

// one block: sums of the partials in a fixed order, then the CG scalars
__global__ void __launch_bounds__(BLOCK) k_fin(const double *partA, const double *partB, int nb, double *sc, int op)
{
    __shared__ double sh[BLOCK];
    double a = 0.0, bsum = 0.0;
    for (int k = threadIdx.x; k < nb; k += BLOCK) {
        a += partA[k];
        if (partB) bsum += partB[k];
    }
    a = block_sum(a, sh);
    if (partB) bsum = block_sum(bsum, sh);
    if (threadIdx.x != 0) return;
    if (op == FIN_ALPHA) {                            // a = p.q
        sc[SC_PQ] = a;
        sc[SC_ALPHA] = a != 0.0 ? sc[SC_RZ] / a : 0.0;
    } else {                                          // a = r.r, bsum = r.z (no preconditioner: z = r)
        const double rz = partB ? bsum : a;
        sc[SC_RR] = a;
        sc[SC_BETA] = (op == FIN_BETA && sc[SC_RZ] != 0.0) ? rz / sc[SC_RZ] : 0.0;
        sc[SC_RZ] = rz;
    }
}

// x += alpha p; r -= alpha q; (Jacobi: z = dinv r); partials of r.r and r.z
__global__ void __launch_bounds__(BLOCK) k_update(long long n, double *x, double *r, const double *p, const double *q,
                                                  const double *dinv, double *z, const double *sc, double *partA, double *partB)
{
    __shared__ double sh[BLOCK];
    const double alpha = sc[SC_ALPHA];
    double rr = 0.0, rz = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * q[i];
        r[i] = ri;
        rr += ri * ri;
        if (dinv) {
            const double zi = dinv[i] * ri;
            z[i] = zi;
            rz += ri * zi;
        }
    }
    rr = block_sum(rr, sh);
    if (threadIdx.x == 0) partA[blockIdx.x] = rr;
    if (dinv) {
        rz = block_sum(rz, sh);
        if (threadIdx.x == 0) partB[blockIdx.x] = rz;
    }
}

__global__ void k_pupdate(long long n, const double *z, double *p, const double *sc)
{
    const double beta = sc[SC_BETA];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        p[i] = z[i] + beta * p[i];
}

// ---------------------------------------------------------------------------------------------
// BiCGStab (right-preconditioned, the "Templates" variant).  Its scalars live in a block of their own (BS_*)
// that only k_fin_bicg writes.  BS_DONE freezes the solve: every update kernel returns at once when it is set, so iterations run
// past the stop (check_every > 1) change neither x nor r.  BS_LAST marks the x / r update of this iteration as the final one
// (||s|| small enough, or omega broke down: x += alpha p^, r = s); the next FB_RHO then sets BS_DONE.  BS_RESTART makes k_bicg_p
// start afresh from the current residual (r^ = p = r).
enum { BS_RHO = 0, BS_RHO_OLD, BS_ALPHA, BS_OMEGA, BS_BETA, BS_RR, BS_IT, BS_DONE, BS_LAST, BS_CONV, BS_REASON, BS_RESTART,
       BS_RESTART_IT, BS_NRESTART, BS_N = 16 };
enum { FB_INIT = 0, FB_RHO, FB_ALPHA, FB_S, FB_OMEGA };
// Breakdown.  rho = r^.r is zero once it has cancelled to below BICG_EPS_RHO times the sum of the magnitudes of its terms (scipy's
// eps^2, made independent of the scale): the iteration restarts with r^ = p = r, and stops (IGX_BREAKDOWN_RHO) only if rho
// vanishes again in the iteration right after a restart.  r^.v is zero when the step it gives is absurd:
// BICG_EPS_ALPHA |alpha| ||v|| > ||r||.
// (Near-breakdowns that BiCGStab survives -- r^.v cancelled to 1e-16 of its terms with a step of 200 ||r|| on the convection-
// dominated notebook problem -- pass; a skew-symmetric R A R^T, where r0.A r0 = 0, stops in its first iteration.)
constexpr double BICG_EPS_RHO = 2.220446049250313e-16 * 2.220446049250313e-16;
constexpr double BICG_EPS_ALPHA = 1e-13;

__device__ __forceinline__ bool is_fin(double v) { return v - v == 0.0; }

// one block: sums of the partials in a fixed order (partA: nA of them, partB and partC: nB), then the BiCGStab scalars of step `op`
__global__ void __launch_bounds__(BLOCK) k_fin_bicg(const double *partA, int nA, const double *partB, int nB, const double *partC,
                                                    double *sc, int op, double stop)
{
    __shared__ double sh[BLOCK];
    if (sc[BS_DONE] != 0.0) return;                               // (uniform: nothing below changes once stopped)
    double a = 0.0, bsum = 0.0, csum = 0.0;
    for (int k = threadIdx.x; k < nA; k += BLOCK) a += partA[k];
    for (int k = threadIdx.x; k < nB; k += BLOCK) {
        bsum += partB[k];
        if (partC) csum += partC[k];
    }
    a = block_sum(a, sh);
    if (partB) bsum = block_sum(bsum, sh);
    if (partC) csum = block_sum(csum, sh);
    if (threadIdx.x != 0) return;
    auto halt = [&](int conv, int reason) { sc[BS_DONE] = 1.0; sc[BS_CONV] = conv; if (reason) sc[BS_REASON] = reason; };
    switch (op) {
    case FB_INIT:                                                 // a = r.r (r^ = r)
        bsum = csum = a;
        [[fallthrough]];
    case FB_RHO: {                                                // a = r.r, bsum = r^.r, csum = sum |r^_i r_i|
        const double rr = a, rho = bsum;
        sc[BS_RR] = rr;
        if (sc[BS_LAST] != 0.0) { sc[BS_DONE] = 1.0; return; }   // (BS_CONV / BS_REASON set with BS_LAST)
        if (!is_fin(rr) || !is_fin(rho)) { halt(0, IGX_BREAKDOWN_NONFINITE); return; }
        if (sqrt(rr) <= stop) { halt(1, 0); return; }
        if (fabs(rho) <= BICG_EPS_RHO * csum) {
            if (sc[BS_NRESTART] > 0.0 && sc[BS_RESTART_IT] == sc[BS_IT] - 1.0) { halt(0, IGX_BREAKDOWN_RHO); return; }
            sc[BS_RESTART] = 1.0;                                 // r^ = p = r: rho = r.r
            sc[BS_RESTART_IT] = sc[BS_IT];
            sc[BS_NRESTART] += 1.0;
            sc[BS_BETA] = 0.0;
            sc[BS_RHO] = sc[BS_RHO_OLD] = rr;
            return;
        }
        const double beta = sc[BS_IT] > 0.0 ? (rho / sc[BS_RHO_OLD]) * (sc[BS_ALPHA] / sc[BS_OMEGA]) : 0.0;
        if (!is_fin(beta)) { halt(0, IGX_BREAKDOWN_NONFINITE); return; }
        sc[BS_BETA] = beta;
        sc[BS_RHO] = sc[BS_RHO_OLD] = rho;
        return;
    }
    case FB_ALPHA: {                                              // a = r^.v
        sc[BS_IT] += 1.0;                                         // an iteration is entered at its first SpMV
        sc[BS_RESTART] = 0.0;
        const double alpha = sc[BS_RHO] / a;
        if (!is_fin(a) || !is_fin(alpha)) { halt(0, a == 0.0 ? IGX_BREAKDOWN_ALPHA : IGX_BREAKDOWN_NONFINITE); return; }
        sc[BS_ALPHA] = alpha;
        return;
    }
    case FB_S: {                                                  // a = s.s, bsum = v.v
        if (!is_fin(a) || !is_fin(bsum)) { halt(0, IGX_BREAKDOWN_NONFINITE); return; }
        if (BICG_EPS_ALPHA * fabs(sc[BS_ALPHA]) * sqrt(bsum) > sqrt(sc[BS_RR])) { halt(0, IGX_BREAKDOWN_ALPHA); return; }
        if (sqrt(a) <= stop) { sc[BS_LAST] = 1.0; sc[BS_CONV] = 1.0; }
        return;
    }
    default: {                                                    // FB_OMEGA: a = t.s, bsum = t.t
        if (sc[BS_LAST] != 0.0) { sc[BS_OMEGA] = 0.0; return; }
        const double omega = a / bsum;
        if (!is_fin(omega) || omega == 0.0) {                     // (t.t == 0 included) keep the half step x + alpha p^ and stop
            sc[BS_OMEGA] = 0.0;
            sc[BS_LAST] = 1.0;
            sc[BS_REASON] = is_fin(a) && is_fin(bsum) ? IGX_BREAKDOWN_OMEGA : IGX_BREAKDOWN_NONFINITE;
            return;
        }
        sc[BS_OMEGA] = omega;
        return;
    }
    }
}

// p = r + beta (p - omega v), or r^ = p = r on a restart; (Jacobi: ph = dinv p)
__global__ void k_bicg_p(long long n, const double *r, double *p, const double *v, const double *dinv, double *ph, double *rh,
                         const double *sc)
{
    if (sc[BS_DONE] != 0.0) return;
    const double beta = sc[BS_BETA], omega = sc[BS_OMEGA];
    const bool restart = sc[BS_RESTART] != 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double pi = restart ? r[i] : r[i] + beta * (p[i] - omega * v[i]);
        if (restart) rh[i] = pi;
        p[i] = pi;
        if (dinv) ph[i] = dinv[i] * pi;
    }
}

// s = r - alpha v; (Jacobi: sh = dinv s); partials of s.s and v.v
__global__ void __launch_bounds__(BLOCK) k_bicg_s(long long n, const double *r, const double *v, double *s, const double *dinv, double *sh_,
                                                  const double *sc, double *partA, double *partB)
{
    __shared__ double sh[BLOCK];
    if (sc[BS_DONE] != 0.0) return;
    const double alpha = sc[BS_ALPHA];
    double ss = 0.0, vv = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        const double vi = v[i], si = r[i] - alpha * vi;
        s[i] = si;
        if (dinv) sh_[i] = dinv[i] * si;
        ss += si * si;
        vv += vi * vi;
    }
    ss = block_sum(ss, sh);
    vv = block_sum(vv, sh);
    if (threadIdx.x == 0) { partA[blockIdx.x] = ss; partB[blockIdx.x] = vv; }
}

// x += alpha ph [+ omega sh]; r = s [- omega t]; partials of r.r, r^.r and sum |r^_i r_i|
__global__ void __launch_bounds__(BLOCK) k_bicg_xr(long long n, double *x, double *r, const double *ph, const double *sh_, const double *s,
                                                   const double *t, const double *rh, const double *sc, double *partA, double *partB,
                                                   double *partC)
{
    __shared__ double sh[BLOCK];
    if (sc[BS_DONE] != 0.0) return;
    const double alpha = sc[BS_ALPHA], omega = sc[BS_OMEGA];
    double rr = 0.0, rhr = 0.0, arhr = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        double xi = x[i] + alpha * ph[i], ri = s[i];
        if (omega != 0.0) { xi += omega * sh_[i]; ri -= omega * t[i]; }     // (omega = 0: the half step; sh, t are not read)
        x[i] = xi;
        r[i] = ri;
        const double q = rh[i] * ri;
        rr += ri * ri;
        rhr += q;
        arhr += fabs(q);
    }
    rr = block_sum(rr, sh);
    rhr = block_sum(rhr, sh);
    arhr = block_sum(arhr, sh);
    if (threadIdx.x == 0) { partA[blockIdx.x] = rr; partB[blockIdx.x] = rhr; partC[blockIdx.x] = arhr; }
}

// ---------------------------------------------------------------------------------------------
// Kronecker contraction of tensor dim kd (of 4: three spatial axes + a trailing batch axis):
//     Y[..., i, ...] = (sum_j B[i][j] X[..., j, ...]) [ / D(i0, i1, i2) ]
// A GEMM of B (m x n) with the matrix X whose columns are the other three tensor indices (C order).  Tile 64 x 64 of (i, column),
// TK values of j per LDS step (the next step's tile is loaded into registers meanwhile), 4 x 4 results per thread.
constexpr int TM = 64, TN = 64, TK = 32, LPT = TK * TN / 256;     // LPT: values of each tile every thread loads

struct KStep {
    const double *B;
    int m, n, kd;
    int ext[4];                          // extents of the other dims (ext[kd] unused)
    long long sx[4], sy[4], xoff, yoff;
    long long ncol;
    int lam_mode;                        // 0: none, 1: divide by sum_k lam[k][i_k], 2: by the product
    const double *lam[3];
};

__device__ __forceinline__ void col_index(const KStep &S, long long col, int idx[4])
{
#pragma unroll
    for (int d = 3; d >= 0; --d) {
        if (d == S.kd) { idx[d] = 0; continue; }
        idx[d] = (int)(col % S.ext[d]);
        col /= S.ext[d];
    }
}

template <bool JFAST>
__global__ void __launch_bounds__(256) k_kron(const KStep S, const double *__restrict__ X, double *__restrict__ Y)
{
    __shared__ double Bs[TK][TM + 1];
    __shared__ double Xs[TK][TN + 1];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const long long c0 = (long long)blockIdx.x * TN;
    const int i0 = blockIdx.y * TM;
    const long long sxk = S.sx[S.kd];
    // tile element l of this thread: B (kb, ib) and X (kx, cx).  JFAST (unit stride along j): LPT columns, one j each; else one
    // column, LPT values of j
    long long loff[LPT];
    bool lok[LPT];
#pragma unroll
    for (int l = 0; l < LPT; ++l) {
        const long long col = c0 + (JFAST ? (t / TK + (256 / TK) * l) : (t % TN));
        int idx[4];
        lok[l] = col < S.ncol;
        col_index(S, lok[l] ? col : 0, idx);
        loff[l] = S.xoff + idx[0] * S.sx[0] + idx[1] * S.sx[1] + idx[2] * S.sx[2] + idx[3] * S.sx[3];
    }
    double rb[LPT], rx[LPT];
    auto load = [&](int k0) {
#pragma unroll
        for (int l = 0; l < LPT; ++l) {
            const int i = i0 + t / TK + (256 / TK) * l, j = k0 + t % TK;
            rb[l] = (i < S.m && j < S.n) ? S.B[(long long)i * S.n + j] : 0.0;
            const int jx = k0 + (JFAST ? t % TK : t / TN + (256 / TN) * l);
            rx[l] = (lok[l] && jx < S.n) ? X[loff[l] + jx * sxk] : 0.0;
        }
    };
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    load(0);
    for (int k0 = 0; k0 < S.n; k0 += TK) {
#pragma unroll
        for (int l = 0; l < LPT; ++l) {
            Bs[t % TK][t / TK + (256 / TK) * l] = rb[l];
            if (JFAST) Xs[t % TK][t / TK + (256 / TK) * l] = rx[l];
            else Xs[t / TN + (256 / TN) * l][t % TN] = rx[l];
        }
        __syncthreads();
        if (k0 + TK < S.n) load(k0 + TK);             // the next tile is in flight while this one is used
#pragma unroll 8
        for (int k = 0; k < TK; ++k) {
            double a[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = Bs[k][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) bv[c] = Xs[k][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], bv[c], acc[r][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const long long col = c0 + tx + 16 * c;
        if (col >= S.ncol) continue;
        int idx[4];
        col_index(S, col, idx);
        const long long yo = S.yoff + idx[0] * S.sy[0] + idx[1] * S.sy[1] + idx[2] * S.sy[2] + idx[3] * S.sy[3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + ty + 16 * r;
            if (i >= S.m) continue;
            double v = acc[r][c];
            if (S.lam_mode) {
                double d = S.lam_mode == 1 ? 0.0 : 1.0;
                for (int e = 0; e < 3; ++e) {
                    if (!S.lam[e]) continue;
                    const double l = S.lam[e][e == S.kd ? i : idx[e]];
                    d = S.lam_mode == 1 ? d + l : d * l;
                }
                v /= d;
            }
            Y[yo + (long long)i * S.sy[S.kd]] = v;
        }
    }
}

long long kron_work_len(const KronPlan &P)         // doubles of ONE of the two work buffers
{
    long long mx = 0;
    for (int k = 0; k + 1 < P.dim; ++k) {
        long long s = P.batch;
        for (int e = 0; e < P.dim; ++e) s *= e <= k ? P.m[e] : P.n[e];
        mx = std::max(mx, s);
    }
    return mx;
}

// work: two buffers of kron_work_len doubles; with dim >= 2 step k writes W[k % 2], so the last step reads W[dim % 2]
int launch_kron_plan(hipStream_t st, const KronPlan &P, const double *x, double *y, double *const W[2])
{
    int cur[4] = {1, 1, 1, (int)P.batch};           // extents of the current tensor
    for (int e = 0; e < P.dim; ++e) cur[e] = P.n[e];
    for (int k = 0; k < P.dim; ++k) {
        KStep S{};
        S.B = P.B[k]; S.m = P.m[k]; S.n = P.n[k]; S.kd = k;
        for (int e = 0; e < 4; ++e) S.ext[e] = cur[e];
        S.ncol = 1;
        for (int e = 0; e < 4; ++e)
            if (e != k) S.ncol *= cur[e];
        const bool first = k == 0, last = k == P.dim - 1;
        // compact C-order strides of an intermediate (input: extents cur, output: cur with m[k] at k)
        long long cs_in[4], cs_out[4];
        {
            int out[4] = {cur[0], cur[1], cur[2], cur[3]};
            out[k] = P.m[k];
            long long a = 1, b = 1;
            for (int e = 3; e >= 0; --e) { cs_in[e] = a; a *= cur[e]; cs_out[e] = b; b *= out[e]; }
        }
        const double *src = first ? x : W[(k - 1) % 2];
        double *dst = last ? y : W[k % 2];
        for (int e = 0; e < 4; ++e) {
            S.sx[e] = first ? P.x_stride[e] : cs_in[e];
            S.sy[e] = last ? P.y_stride[e] : cs_out[e];
        }
        S.xoff = first ? P.x_off : 0;
        S.yoff = last ? P.y_off : 0;
        S.lam_mode = last ? P.lam_mode : 0;
        for (int e = 0; e < 3; ++e) S.lam[e] = (last && e < P.dim) ? P.lam[e] : nullptr;
        if (S.ncol > 0 && S.m > 0) {
            const long long gx = (S.ncol + TN - 1) / TN;
            if (gx > 0x7fffffffLL) { set_error("Kronecker apply: %lld column tiles", gx); return IGX_ERR_UNSUPPORTED; }
            dim3 grid((unsigned)gx, (unsigned)((S.m + TM - 1) / TM));
            if (S.sx[k] == 1) k_kron<true><<<grid, 256, 0, st>>>(S, src, dst);
            else k_kron<false><<<grid, 256, 0, st>>>(S, src, dst);
            IGX_HIP(hipGetLastError());
        }
        cur[k] = P.m[k];
    }
    return IGX_OK;
}

int spmv_gw(long long maxlen)
{
    return maxlen >= 192 ? 64 : maxlen >= 96 ? 32 : maxlen >= 48 ? 16 : maxlen >= 24 ? 8 : 4;
}

// f(the instantiation of the structured / CSR SpMV at group width gw): the only place that names one, so that the occupancy
// query and the launch cannot take different kernels
template <class F>
decltype(auto) with_spmv_kernel(int gw, F &&f)
{
    switch (gw) {
    case 64: return f(k_spmv<64, 12>);
    case 32: return f(k_spmv<32, 4>);
    case 16: return f(k_spmv<16, 4>);
    case 8: return f(k_spmv<8, 4>);
    default: return f(k_spmv<4, 4>);
    }
}

template <class F>
decltype(auto) with_csr_spmv_kernel(int gw, F &&f)
{
    switch (gw) {
    case 64: return f(k_csr_spmv<64, 8>);
    case 32: return f(k_csr_spmv<32, 4>);
    case 16: return f(k_csr_spmv<16, 4>);
    case 8: return f(k_csr_spmv<8, 4>);
    default: return f(k_csr_spmv<4, 4>);
    }
}

// the same for the block SpMV of nc = 2 or 3 components (U: NC^2 U values of each lane in flight)
template <class F>
decltype(auto) with_block_spmv_kernel(int gw, int nc, F &&f)
{
    if (nc == 3) {
        switch (gw) {
        case 64: return f(k_block_spmv<64, 2, 3>);
        case 32: return f(k_block_spmv<32, 2, 3>);
        case 16: return f(k_block_spmv<16, 2, 3>);
        case 8: return f(k_block_spmv<8, 2, 3>);
        default: return f(k_block_spmv<4, 2, 3>);
        }
    }
    switch (gw) {
    case 64: return f(k_block_spmv<64, 4, 2>);
    case 32: return f(k_block_spmv<32, 4, 2>);
    case 16: return f(k_block_spmv<16, 4, 2>);
    case 8: return f(k_block_spmv<8, 4, 2>);
    default: return f(k_block_spmv<4, 4, 2>);
    }
}

// the same for the block SpMV over a multipatch's CSR pattern (the U of k_block_spmv: the same NC^2 U values in flight per lane)
template <class F>
decltype(auto) with_csr_block_spmv_kernel(int gw, int nc, F &&f)
{
    if (nc == 3) {
        switch (gw) {
        case 64: return f(k_csr_block_spmv<64, 2, 3>);
        case 32: return f(k_csr_block_spmv<32, 2, 3>);
        case 16: return f(k_csr_block_spmv<16, 2, 3>);
        case 8: return f(k_csr_block_spmv<8, 2, 3>);
        default: return f(k_csr_block_spmv<4, 2, 3>);
        }
    }
    switch (gw) {
    case 64: return f(k_csr_block_spmv<64, 4, 2>);
    case 32: return f(k_csr_block_spmv<32, 4, 2>);
    case 16: return f(k_csr_block_spmv<16, 4, 2>);
    case 8: return f(k_csr_block_spmv<8, 4, 2>);
    default: return f(k_csr_block_spmv<4, 4, 2>);
    }
}

// ---------------------------------------------------------------------------------------------
// the fast-diagonalization inverse of one box (FastDiag, solve_internal.h)

// C-order strides of a compact box vector
void box_strides(int dim, const int *m, long long stride[4])
{
    for (int k = 0; k < 4; ++k) stride[k] = 1;
    for (int k = dim - 2; k >= 0; --k) stride[k] = stride[k + 1] * m[k + 1];
}

// appends the factors of one box to h (U[k]: m[k] x m[k] row-major, lam[k]: m[k]); returns the offset they start at
size_t pack_fastdiag(std::vector<double> &h, int dim, const int *m, const double *const *U, const double *const *lam)
{
    const size_t at = h.size();
    for (int k = 0; k < dim; ++k) {
        const size_t mk = (size_t)m[k], o = h.size();
        h.resize(o + 2 * mk * mk + mk);
        for (size_t a = 0; a < mk; ++a)
            for (size_t b = 0; b < mk; ++b) h[o + a * mk + b] = U[k][b * mk + a];
        std::memcpy(&h[o + mk * mk], U[k], mk * mk * sizeof(double));
        std::memcpy(&h[o + 2 * mk * mk], lam[k], mk * sizeof(double));
    }
    return at;
}

// the two plans of a box over its packed factors `fac` (on the device); batch > 1: blocks of `batch` interleaved columns
// (entry (I, j) at I * batch + j), the trailing batch axis of k_kron
FastDiag make_fastdiag(int dim, const int *m, const double *fac, const long long io_stride[4], long long io_off, int lam_mode,
                       long long batch = 1)
{
    FastDiag F{};
    F.dim = dim;
    KronPlan &L = F.kl, &R = F.kr;
    L.dim = R.dim = dim;
    L.batch = R.batch = batch;
    long long box_stride[4];
    box_strides(dim, m, box_stride);
    for (int k = 0; k < 3; ++k) {
        L.x_stride[k] = R.y_stride[k] = (k < dim ? io_stride[k] : 1) * batch;
        L.y_stride[k] = R.x_stride[k] = box_stride[k] * batch;
    }
    L.x_stride[3] = R.y_stride[3] = L.y_stride[3] = R.x_stride[3] = 1;
    L.x_off = R.y_off = io_off * batch;
    for (int k = 0; k < dim; ++k) {
        const size_t mk = (size_t)m[k];
        L.m[k] = L.n[k] = R.m[k] = R.n[k] = m[k];
        L.B[k] = fac;
        R.B[k] = fac + mk * mk;
        L.lam[k] = fac + 2 * mk * mk;
        fac += 2 * mk * mk + mk;
    }
    L.lam_mode = lam_mode;
    return F;
}

} // namespace

// the host side: what solve_internal.h declares is called by the other units as well, what is static by this one only
namespace igx {

// y = F x with two work buffers of a box each.  With dim >= 2 step k of a plan writes W[k % 2]: the compact result t of the first
// product goes where its last step does not write, and the second product alternates between the other buffer and t, so that
// its step 0 does not write t, which it reads
int apply_fastdiag(hipStream_t st, const FastDiag &F, const double *x, double *y, double *const W[2])
{
    double *t = W[(F.dim - 1) % 2];
    if (int rc = launch_kron_plan(st, F.kl, x, t, W)) return rc;
    double *W2[2] = {W[F.dim % 2], t};
    return launch_kron_plan(st, F.kr, t, y, W2);
}

int spmv_group_width(long long maxlen) { return spmv_gw(maxlen); }

void mask_copy(hipStream_t st, const igx_solver *s, const double *x, double *y)
{
    k_mask_copy<<<(unsigned)((s->n + 255) / 256), 256, 0, st>>>(s->n, s->d_mask, x, y);
}

void jacobi_diagonal(hipStream_t st, const igx_solver *s, const double *vals, double *dinv, int comp)
{
    if (const igx_multipatch *m = s->mp) {
        const long long N = m->nglobal;
        k_csr_diag<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(N, m->d_indptr, m->d_indices, vals, s->d_mask + comp * N, dinv);
        return;
    }
    const long long N = s->g.nrows;
    k_diag<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(s->g, vals, s->d_mask + comp * N, dinv);
}

int sum_partials(hipStream_t st, igx_solver *s, unsigned nb, double *sum)
{
    k_fin<<<1, BLOCK, 0, st>>>(s->d_part, nullptr, nb, s->d_sc, FIN_INIT);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipMemcpyAsync(sum, s->d_sc + SC_RR, sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int check_values(const igx_solver *s, const char *what)
{
    if (s->saddle) return saddle_check_values(s, what);
    if (s->ncomp > 1) {                       // (the blocks are the solver's own: only a missing diagonal one is refused)
        for (int c = 0; c < s->ncomp; ++c)
            if (!s->block.blk[c * s->ncomp + c]) {
                set_error("%s: diagonal block (%d, %d) missing: take it first (%s)", what, c, c,
                          s->mp ? "igx_solver_take_multipatch_block" : "igx_solver_take_block");
                return IGX_ERR_ARG;
            }
        return s->mp && s->precond == IGX_PRECOND_MG ? mg_check(s, what) : IGX_OK;
    }
    if (s->mp) {
        if (s->mp->generation != s->gen) {
            set_error("%s: the multipatch's sums were restarted (igx_multipatch_zero) since the solver was made: make a new solver "
                      "over the new sums", what);
            return IGX_ERR_ARG;
        }
        return s->precond == IGX_PRECOND_MG ? mg_check(s, what) : IGX_OK;     // (every coarser level's sums as well)
    }
    if (s->parabolic) {                       // (its values are its own: they must be taken and C formed)
        if (!s->par.c_formed) {
            set_error("%s: no C = M + tau gamma K yet: take M and K (igx_solver_take_values), then igx_solver_set_dirk", what);
            return IGX_ERR_ARG;
        }
        return IGX_OK;
    }
    if (s->pt->values_kind != s->kind || !s->pt->d_data) {
        set_error("%s: the patch no longer holds the values of the solver's matrix (another kind was assembled since, or an "
                  "assembly failed): assemble it again", what);
        return IGX_ERR_ARG;
    }
    return IGX_OK;
}

// the values a scalar patch solver's SpMV and Jacobi read: the patch's, or a parabolic solver's own C
const double *patch_values(const igx_solver *s)
{
    if (!s->parabolic) return s->pt->d_data;
    return s->par.vals_sel ? s->par.vals_sel : s->par.pv[2];       // (vals_sel: M, during the mass solve of an embedded DIRK attempt)
}

static unsigned spmv_blocks(const igx_solver *s)
{
    const long long groups = BLOCK / s->gw, rows = s->n / s->ncomp;      // (a block solver: one group per scalar row)
    return (unsigned)std::max<long long>(1, std::min<long long>(s->nb_spmv, (rows + groups - 1) / groups));
}

// y = free ? (b ? b : 0) + sign A x : 0 (and the partials of pd.y): k_spmv on a patch's values, k_csr_spmv on a multipatch's sums,
// k_block_spmv on the blocks of a block solver, k_csr_block_spmv on those of a multipatch block solver
int spmv(hipStream_t st, const igx_solver *s, const double *x, const double *b, double sign, double *y, const double *pd, double *part)
{
    if (s->saddle) return saddle_spmv(st, s, x, b, sign, y, pd, part);
    const unsigned nb = spmv_blocks(s);
    if (s->mp && s->ncomp > 1) {
        const igx_multipatch *m = s->mp;
        BlockVals A{};
        for (int k = 0; k < s->ncomp * s->ncomp; ++k) A.v[k] = s->block.blk[k];
        with_csr_block_spmv_kernel(s->gw, s->ncomp, [&](auto k) {
            k<<<nb, BLOCK, 0, st>>>(m->nglobal, m->d_indptr, m->d_indices, A, s->d_mask, x, b, sign, y, pd, part);
        });
    } else if (s->mp) {
        const igx_multipatch *m = s->mp;
        with_csr_spmv_kernel(s->gw, [&](auto k) {
            k<<<nb, BLOCK, 0, st>>>(s->n, m->d_indptr, m->d_indices, m->d_vals, s->d_mask, x, b, sign, y, pd, part);
        });
    } else if (s->ncomp > 1) {
        BlockVals A{};
        for (int k = 0; k < s->ncomp * s->ncomp; ++k) A.v[k] = s->block.blk[k];
        with_block_spmv_kernel(s->gw, s->ncomp, [&](auto k) { k<<<nb, BLOCK, 0, st>>>(s->g, A, s->d_mask, x, b, sign, y, pd, part); });
    } else {
        const double *vals = patch_values(s);
        with_spmv_kernel(s->gw, [&](auto k) { k<<<nb, BLOCK, 0, st>>>(s->g, vals, s->d_mask, x, b, sign, y, pd, part); });
    }
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

// k_spmv over other values of the same layout (a parabolic solver's M or K): y = free ? (b ? b : 0) + sign V x : 0
int spmv_values(hipStream_t st, const igx_solver *s, const double *vals, const double *x, const double *b, double sign, double *y)
{
    const unsigned nb = spmv_blocks(s);
    with_spmv_kernel(s->gw, [&](auto k) { k<<<nb, BLOCK, 0, st>>>(s->g, vals, s->d_mask, x, b, sign, y, nullptr, nullptr); });
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

unsigned vec_blocks(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>(NB_VEC, (n + BLOCK - 1) / BLOCK)); }

// z = P r on the free box (kron; a block solver: on the free box of every component, diag(P_0, .., P_{nc-1})), or nothing
// (none / Jacobi: z is formed by k_update or is r itself)
static int apply_kron(hipStream_t st, igx_solver *s, const double *r, double *z)
{
    double *W[2] = {s->d_W, s->d_W + s->wlen};
    if (s->ncomp > 1) {
        for (int c = 0; c < s->ncomp; ++c)
            if (int rc = apply_fastdiag(st, s->block.bkron[c], r, z, W)) return rc;
        return IGX_OK;
    }
    return apply_fastdiag(st, s->kron, r, z, W);
}

// z = sum_p X_p M_p B_p M_p X_p^T r: per patch, in patch order, gather the box, the two Kronecker products, add back on the free dofs
// (a multipatch block solver: component after component on its slice of the vectors and of the mask, with its own patches)
static int apply_schwarz(hipStream_t st, igx_solver *s, const double *r, double *z)
{
    IGX_HIP(hipMemsetAsync(z, 0, (size_t)s->n * sizeof(double), st));
    double *W[2] = {s->d_W, s->d_W + s->wlen};
    const long long N = s->n / s->ncomp;
    for (int c = 0; c < s->ncomp; ++c) {
        const long long o = c * N;
        for (const SwPatch &P : s->ncomp > 1 ? s->block.bsw[c] : s->sw) {
            const unsigned nb = (unsigned)((P.map.nbox + 255) / 256);
            k_box_gather<<<nb, 256, 0, st>>>(P.map, s->d_mask + o, r + o, s->d_box);
            IGX_HIP(hipGetLastError());
            if (int rc = apply_fastdiag(st, P.F, s->d_box, s->d_box, W)) return rc;
            k_box_scatter<<<nb, 256, 0, st>>>(P.map, s->d_mask + o, s->d_box, z + o);
            IGX_HIP(hipGetLastError());
        }
    }
    return IGX_OK;
}

// the preconditioners applied by kernels of their own (Kronecker, Schwarz); Jacobi is fused into k_update
static int apply_dense(hipStream_t st, igx_solver *s, const double *r, double *z)
{
    if (s->precond == IGX_PRECOND_MG) return mg_apply(st, s, r, z);
    return s->precond == IGX_PRECOND_SCHWARZ ? apply_schwarz(st, s, r, z) : apply_kron(st, s, r, z);
}

static int spmv_occupancy(const igx_solver *s)
{
    int per_cu = 0;
    auto occupancy = [&](auto k) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, BLOCK, 0); };
    const hipError_t eo = s->mp ? (s->ncomp > 1 ? with_csr_block_spmv_kernel(s->gw, s->ncomp, occupancy) : with_csr_spmv_kernel(s->gw, occupancy))
                                : s->ncomp > 1 ? with_block_spmv_kernel(s->gw, s->ncomp, occupancy) : with_spmv_kernel(s->gw, occupancy);
    if (eo != hipSuccess) { (void)hipGetLastError(); per_cu = 1; }
    return (int)std::min<long long>(NB_SPMV_MAX, (long long)std::max(1, per_cu) * std::max(1, s->ctx->ncu));
}

void free_solver(igx_solver *s)
{
    mg_free(s);
    eig_free(s);
    s->bicg.release(); s->block.release(); s->par.release(); s->step.release(); s->sad.release(); s->gm.release();
    (void)hipFree(s->d_tab); (void)hipFree(s->d_mask); (void)hipFree(s->d_vec); (void)hipFree(s->d_part); (void)hipFree(s->d_sc);
    (void)hipFree(s->d_kron); (void)hipFree(s->d_W); (void)hipFree(s->d_box);
    if (s->have_ev)
        for (auto &e : s->ev) (void)hipEventDestroy(e);
    delete s;
}

// the dof mask from the fixed list (s->n set); false with igx_last_error on a bad list
static bool set_fixed(igx_solver *s, const int64_t *fixed, int64_t nfixed, const char *what)
{
    s->h_free.assign((size_t)s->n, 1);
    for (int64_t k = 0; k < nfixed; ++k) {
        if (fixed[k] < 0 || fixed[k] >= s->n) { set_error("%s: fixed dof %lld out of range", what, (long long)fixed[k]); return false; }
        if (!s->h_free[fixed[k]]) { set_error("%s: fixed dof %lld given twice", what, (long long)fixed[k]); return false; }
        s->h_free[fixed[k]] = 0;
        s->fixed.push_back(fixed[k]);
    }
    return true;
}

// the dof mask on the device, the CG vectors, partial sums, scalars and events (s->n, s->h_free set)
static int init_vectors(igx_solver *s, const char *what)
{
    const size_t n = (size_t)s->n;
    bool ok = hipMalloc((void **)&s->d_mask, n) == hipSuccess &&
              hipMalloc((void **)&s->d_vec, 8 * n * sizeof(double)) == hipSuccess &&
              hipMalloc((void **)&s->d_part, 2 * (size_t)NB_SPMV_MAX * sizeof(double)) == hipSuccess &&
              hipMalloc((void **)&s->d_sc, SC_N * sizeof(double)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); set_error("%s: out of device memory (%.3f GB)", what, 8.0 * 8 * n / 1e9); return IGX_ERR_NOMEM; }
    hipStream_t st = s->ctx->stream;
    hipError_t e = hipMemcpyAsync(s->d_mask, s->h_free.data(), n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_vec, 0, 8 * n * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_sc, 0, SC_N * sizeof(double), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return IGX_ERR_HIP; }
    double *v = s->d_vec;
    s->x = v; s->r = v + n; s->p = v + 2 * n; s->q = v + 3 * n; s->z = v + 4 * n; s->b = v + 5 * n; s->w = v + 6 * n; s->dinv = v + 7 * n;
    for (auto &ev : s->ev)
        if (hipEventCreate(&ev) != hipSuccess) { set_error("%s: hipEventCreate failed", what); return IGX_ERR_HIP; }
    s->have_ev = true;
    return IGX_OK;
}

// the BiCGStab vectors, scalars and events of a solver (once; a CG-only solver never has them)
int init_bicgstab(igx_solver *s, const char *what)
{
    BicgState &B = s->bicg;
    if (B.d_bvec) return IGX_OK;
    const size_t n = (size_t)s->n;
    if (hipMalloc((void **)&B.d_bvec, 4 * n * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&B.d_bsc, BS_N * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(B.d_bvec); B.d_bvec = nullptr;
        set_error("%s: out of device memory (%.3f GB)", what, 4.0 * 8 * n / 1e9);
        return IGX_ERR_NOMEM;
    }
    hipError_t e = hipMemsetAsync(B.d_bvec, 0, 4 * n * sizeof(double), s->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return IGX_ERR_HIP; }
    B.rh = B.d_bvec; B.sv = B.d_bvec + n; B.sh = B.d_bvec + 2 * n; B.t = B.d_bvec + 3 * n;
    for (auto &ev : B.bev)
        if (hipEventCreate(&ev) != hipSuccess) { set_error("%s: hipEventCreate failed", what); return IGX_ERR_HIP; }
    B.have_bev = true;
    return IGX_OK;
}

// h (packed fast-diagonalization factors, raw eigenvalues) on the device at d_buf, in place of the buffer there; not synchronised
int upload_replacing(hipStream_t st, const std::vector<double> &h, double *&d_buf)
{
    (void)hipFree(d_buf); d_buf = nullptr;
    IGX_HIP(hipMalloc((void **)&d_buf, h.size() * sizeof(double)));
    IGX_HIP(hipMemcpyAsync(d_buf, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st));
    return IGX_OK;
}

// two work buffers of wlen doubles (s->d_W), in place of the previous ones
int alloc_fastdiag_work(igx_solver *s, long long wlen)
{
    (void)hipFree(s->d_W); s->d_W = nullptr; s->wlen = 0;
    IGX_HIP(hipMalloc((void **)&s->d_W, 2 * (size_t)wlen * sizeof(double)));
    s->wlen = wlen;
    return IGX_OK;
}

// Preconditioned CG on R A R^T x = r0 (r0 in s->r, ||R (b - A ext(g))|| = bnorm).  Per iteration: q = A p (and p.q), alpha,
// x += alpha p, r -= alpha q (Jacobi: z = dinv r, fused), z = P r (Kronecker / Schwarz), beta, p = z + beta p.  alpha and beta
// are formed on the device by k_fin; the host reads r.r back every check_every iterations to decide whether to go on.
static int solve_cg(hipStream_t st, igx_solver *s, double bnorm, double tol, int maxiter, int check_every, int timed, igx_solve_info &inf)
{
    const long long n = s->n;
    const unsigned nbv = vec_blocks(n), nbs = spmv_blocks(s);
    double *pA = s->d_part, *pB = s->d_part + NB_SPMV_MAX;
    const bool kron = s->precond == IGX_PRECOND_KRON || s->precond == IGX_PRECOND_SCHWARZ || s->precond == IGX_PRECOND_MG;
    const bool jac = s->precond == IGX_PRECOND_JACOBI;
    // z = P r, rz, rr; p = z
    const double *zz = (kron || jac) ? s->z : s->r;
    if (jac) {
        IGX_HIP(hipMemsetAsync(s->d_sc + SC_ALPHA, 0, sizeof(double), st));   // k_update with alpha = 0: z = dinv r and the dots
        k_update<<<nbv, BLOCK, 0, st>>>(n, s->x, s->r, s->p, s->q, s->dinv, s->z, s->d_sc, pA, pB);
    } else {
        if (kron) {
            if (int rc = apply_dense(st, s, s->r, s->z)) return rc;
        }
        k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->r, s->r, kron ? s->r : nullptr, s->z, pA, pB);
    }
    k_fin<<<1, BLOCK, 0, st>>>(pA, (kron || jac) ? pB : nullptr, nbv, s->d_sc, FIN_INIT);
    k_pupdate<<<nbv, BLOCK, 0, st>>>(n, zz, s->p, s->d_sc);
    IGX_HIP(hipGetLastError());
    double h_rr = 0.0;
    IGX_HIP(hipMemcpyAsync(&h_rr, s->d_sc + SC_RR, sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    const double stop = tol * bnorm;
    bool conv = std::sqrt(h_rr) <= stop;
    int it = 0;
    while (!conv && it < maxiter) {
        ++it;
        if (timed) IGX_HIP(hipEventRecord(s->ev[0], st));
        if (int rc = spmv(st, s, s->p, nullptr, 1.0, s->q, s->p, pA)) return rc;
        if (timed) IGX_HIP(hipEventRecord(s->ev[1], st));
        k_fin<<<1, BLOCK, 0, st>>>(pA, nullptr, nbs, s->d_sc, FIN_ALPHA);
        k_update<<<nbv, BLOCK, 0, st>>>(n, s->x, s->r, s->p, s->q, jac ? s->dinv : nullptr, s->z, s->d_sc, pA, pB);
        IGX_HIP(hipGetLastError());
        if (timed) IGX_HIP(hipEventRecord(s->ev[2], st));
        if (kron) {
            if (int rc = apply_dense(st, s, s->r, s->z)) return rc;
        }
        if (timed) IGX_HIP(hipEventRecord(s->ev[3], st));
        if (kron) k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->r, s->z, nullptr, nullptr, pB, nullptr);
        k_fin<<<1, BLOCK, 0, st>>>(pA, (kron || jac) ? pB : nullptr, nbv, s->d_sc, FIN_BETA);
        k_pupdate<<<nbv, BLOCK, 0, st>>>(n, zz, s->p, s->d_sc);
        IGX_HIP(hipGetLastError());
        if (timed) IGX_HIP(hipEventRecord(s->ev[4], st));
        if (timed || it % check_every == 0 || it == maxiter) {
            IGX_HIP(hipMemcpyAsync(&h_rr, s->d_sc + SC_RR, sizeof(double), hipMemcpyDeviceToHost, st));
            IGX_HIP(hipStreamSynchronize(st));
            conv = std::sqrt(h_rr) <= stop;
            if (timed) {
                float a = 0, b2 = 0, c = 0, d2 = 0;
                (void)hipEventElapsedTime(&a, s->ev[0], s->ev[1]);
                (void)hipEventElapsedTime(&b2, s->ev[1], s->ev[2]);
                (void)hipEventElapsedTime(&c, s->ev[2], s->ev[3]);
                (void)hipEventElapsedTime(&d2, s->ev[3], s->ev[4]);
                inf.spmv_ms += a; inf.precond_ms += c; inf.vector_ms += b2 + d2;
            }
        }
    }
    inf.iterations = it;
    inf.converged = conv ? 1 : 0;
    inf.relres = bnorm > 0.0 ? std::sqrt(h_rr) / bnorm : 0.0;
    return IGX_OK;
}

// Right-preconditioned BiCGStab on R A R^T x = r0 (r0 = R (b - A ext(g)) - R A R^T x0 in s->r, ||R (b - A ext(g))|| = bnorm).
// Per iteration: p = r + beta (p - omega v), p^ = M p, v = A p^ (and r^.v), s = r - alpha v (and s.s, v.v; Jacobi: s^ = M s),
// s^ = M s, t = A s^ (and t.s), t.t, x += alpha p^ + omega s^, r = s - omega t (and r.r, r^.r).  Every scalar is formed on the
// device by k_fin_bicg; the host reads BS_* back every check_every iterations to decide whether to go on.
static int solve_bicgstab(hipStream_t st, igx_solver *s, double bnorm, double tol, int maxiter, int check_every, int timed, igx_solve_info &inf)
{
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    const unsigned nbv = vec_blocks(n), nbs = spmv_blocks(s);
    double *pA = s->d_part, *pB = s->d_part + NB_SPMV_MAX;
    double *pC = pA + NB_VEC;                    // (vector kernels write at most NB_VEC partials into pA: pC follows them)
    const bool dense = s->precond == IGX_PRECOND_KRON || s->precond == IGX_PRECOND_SCHWARZ, jac = s->precond == IGX_PRECOND_JACOBI;
    double *v = s->q;
    double *ph = (dense || jac) ? s->z : s->p, *sh = (dense || jac) ? s->bicg.sh : s->bicg.sv;
    const double *dinv = jac ? s->dinv : nullptr;
    const double stop = tol * bnorm;
    IGX_HIP(hipMemsetAsync(s->bicg.d_bsc, 0, BS_N * sizeof(double), st));
    IGX_HIP(hipMemsetAsync(s->bicg.sh, 0, nbytes, st));
    IGX_HIP(hipMemsetAsync(s->bicg.t, 0, nbytes, st));
    IGX_HIP(hipMemcpyAsync(s->bicg.rh, s->r, nbytes, hipMemcpyDeviceToDevice, st));       // r^ = r0
    k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->r, s->r, nullptr, nullptr, pA, nullptr);
    k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbv, nullptr, 0, nullptr, s->bicg.d_bsc, FB_INIT, stop);
    IGX_HIP(hipGetLastError());
    double h[BS_N] = {};
    auto readback = [&]() -> int {
        IGX_HIP(hipMemcpyAsync(h, s->bicg.d_bsc, sizeof(h), hipMemcpyDeviceToHost, st));
        IGX_HIP(hipStreamSynchronize(st));
        return IGX_OK;
    };
    if (int rc = readback()) return rc;
    hipEvent_t *E = s->bicg.bev;
    for (int it = 0; h[BS_DONE] == 0.0 && it < maxiter;) {
        ++it;
        if (timed) IGX_HIP(hipEventRecord(E[0], st));
        k_bicg_p<<<nbv, BLOCK, 0, st>>>(n, s->r, s->p, v, dinv, ph, s->bicg.rh, s->bicg.d_bsc);
        IGX_HIP(hipGetLastError());
        if (timed) IGX_HIP(hipEventRecord(E[1], st));
        if (dense) { if (int rc = apply_dense(st, s, s->p, ph)) return rc; }
        if (timed) IGX_HIP(hipEventRecord(E[2], st));
        if (int rc = spmv(st, s, ph, nullptr, 1.0, v, s->bicg.rh, pA)) return rc;
        if (timed) IGX_HIP(hipEventRecord(E[3], st));
        k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbs, nullptr, 0, nullptr, s->bicg.d_bsc, FB_ALPHA, stop);
        k_bicg_s<<<nbv, BLOCK, 0, st>>>(n, s->r, v, s->bicg.sv, dinv, sh, s->bicg.d_bsc, pA, pB);
        k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbv, pB, nbv, nullptr, s->bicg.d_bsc, FB_S, stop);
        IGX_HIP(hipGetLastError());
        if (timed) IGX_HIP(hipEventRecord(E[4], st));
        if (dense) { if (int rc = apply_dense(st, s, s->bicg.sv, sh)) return rc; }
        if (timed) IGX_HIP(hipEventRecord(E[5], st));
        if (int rc = spmv(st, s, sh, nullptr, 1.0, s->bicg.t, s->bicg.sv, pA)) return rc;
        if (timed) IGX_HIP(hipEventRecord(E[6], st));
        k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->bicg.t, s->bicg.t, nullptr, nullptr, pB, nullptr);
        k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbs, pB, nbv, nullptr, s->bicg.d_bsc, FB_OMEGA, stop);
        k_bicg_xr<<<nbv, BLOCK, 0, st>>>(n, s->x, s->r, ph, sh, s->bicg.sv, s->bicg.t, s->bicg.rh, s->bicg.d_bsc, pA, pB, pC);
        k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbv, pB, nbv, pC, s->bicg.d_bsc, FB_RHO, stop);
        IGX_HIP(hipGetLastError());
        if (timed) IGX_HIP(hipEventRecord(E[7], st));
        if (timed || it % check_every == 0 || it == maxiter) {
            if (int rc = readback()) return rc;
            if (timed) {
                float ms[7] = {};
                for (int k = 0; k < 7; ++k) (void)hipEventElapsedTime(&ms[k], E[k], E[k + 1]);
                inf.spmv_ms += ms[2] + ms[5];
                inf.precond_ms += ms[1] + ms[4];
                inf.vector_ms += ms[0] + ms[3] + ms[6];
            }
        }
    }
    inf.iterations = (int)h[BS_IT];
    inf.converged = h[BS_CONV] != 0.0 ? 1 : 0;
    inf.relres = bnorm > 0.0 ? std::sqrt(h[BS_RR]) / bnorm : 0.0;
    s->bicg.breakdown = (int)h[BS_REASON];
    return IGX_OK;
}

static bool spd_kind(int kind) { return kind == IGX_MASS || kind == IGX_STIFFNESS; }

// the argument checks of the igx_solver_create* entry points (*out cleared once it can be)
bool create_args_ok(const void *owner, const int64_t *fixed, int64_t nfixed, igx_solver **out, const char *what)
{
    if (!out) { set_error("%s: null argument", what); return false; }
    *out = nullptr;
    if (!owner || (nfixed > 0 && !fixed) || nfixed < 0) { set_error("%s: null argument", what); return false; }
    return true;
}

// what patch and multipatch solvers share: s (ctx, n and its matrix set) gets its fixed dofs, the group width of its longest row
// `maxlen`, its SpMV grid, the per-axis tables `tab` on the device (patch solvers; empty otherwise) and its vectors.  s is freed
// on failure
static int init_solver(igx_solver *s, const int64_t *fixed, int64_t nfixed, long long maxlen, const std::vector<int> &tab, const char *what)
{
    if (!set_fixed(s, fixed, nfixed, what)) { delete s; return IGX_ERR_ARG; }
    s->gw = spmv_gw(maxlen);
    s->nb_spmv = spmv_occupancy(s);
    if (!tab.empty()) {
        if (hipMalloc((void **)&s->d_tab, tab.size() * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError(); set_error("%s: out of device memory (%.3f GB)", what, 8.0 * 8 * s->n / 1e9); free_solver(s); return IGX_ERR_NOMEM;
        }
        hipError_t e = hipMemcpyAsync(s->d_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s->ctx->stream);
        if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); free_solver(s); return IGX_ERR_HIP; }
    }
    if (int rc = init_vectors(s, what)) { free_solver(s); return rc; }
    return IGX_OK;
}

// a solver over the values of `kind` the patch holds (the kind itself checked by the caller; values_now: they must be there now);
// ncomp > 1: a block solver of ncomp components, whose blocks are taken from the patch later (igx_solver_take_block)
int create_patch_solver(igx_patch *pt, int kind, int ncomp, bool values_now, const int64_t *fixed, int64_t nfixed, igx_solver **out,
                        const char *what, long long extra)
{
    if (pt->boxed || pt->row_lo != 0 || pt->row_hi != pt->nrows_total) {
        set_error("%s: whole patches only (no row slab, no span box)", what);
        return IGX_ERR_UNSUPPORTED;
    }
    if (values_now && (pt->values_kind != kind || !pt->d_data)) {
        set_error("%s: assemble the patch with this kind first (igx_assemble, data_out may be NULL)", what);
        return IGX_ERR_ARG;
    }
    if (hipSetDevice(pt->ctx->device) != hipSuccess) { set_error("%s: hipSetDevice failed", what); return IGX_ERR_HIP; }
    igx_solver *s = new igx_solver;
    s->ctx = pt->ctx; s->pt = pt; s->kind = kind; s->dim = pt->dim; s->ncomp = ncomp; s->n = ncomp * pt->nrows_total + extra;
    for (int k = 0; k < pt->dim; ++k) s->N[k] = pt->ax[k].N;
    // per-axis tables as a 3D layout (2D: a one-dof outer axis in front)
    const int off = 3 - pt->dim;
    std::vector<int> tab;
    size_t pos[3][3];
    long long maxlen = 1;
    for (int a = 0; a < 3; ++a) {
        std::vector<int> lo, hi, rp;
        if (a < off) { lo = {0}; hi = {1}; rp = {0, 1}; s->g.N[a] = 1; }
        else {
            const igx::Axis &A = pt->ax[a - off];
            lo = A.jlo; hi = A.jhi; rp = A.rp; s->g.N[a] = A.N;
            int mc = 0;
            for (int i = 0; i < A.N; ++i) mc = std::max(mc, A.jhi[i] - A.jlo[i]);
            maxlen *= mc;
        }
        pos[a][0] = tab.size(); tab.insert(tab.end(), lo.begin(), lo.end());
        pos[a][1] = tab.size(); tab.insert(tab.end(), hi.begin(), hi.end());
        pos[a][2] = tab.size(); tab.insert(tab.end(), rp.begin(), rp.end());
    }
    if (int rc = init_solver(s, fixed, nfixed, maxlen, tab, what)) return rc;
    for (int a = 0; a < 3; ++a) { s->g.jlo[a] = s->d_tab + pos[a][0]; s->g.jhi[a] = s->d_tab + pos[a][1]; s->g.rp[a] = s->d_tab + pos[a][2]; }
    s->g.S1 = tab[pos[1][2] + s->g.N[1]];
    s->g.S2 = tab[pos[2][2] + s->g.N[2]];
    s->g.nrows = pt->nrows_total;
    *out = s;
    return IGX_OK;
}

// the box lo[k] <= i_k < hi[k] (nb[k] = hi[k] - lo[k] out) must be exactly the free dofs of the component at `base` (a patch
// solver: 0): the fast-diagonalization inverse leaves everything outside it at 0
static int check_free_box(const igx_solver *s, long long base, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                   const double *const *lam, int nb[3], const char *what, const int *N, bool free_is_box)
{
    const int d = s->dim;
    for (int k = 0; k < d; ++k) {
        if (box_lo[k] < 0 || box_hi[k] > N[k] || box_lo[k] >= box_hi[k] || !U[k] || !lam[k]) {
            set_error("%s: bad free box [%d, %d) on axis %d", what, box_lo[k], box_hi[k], k);
            return IGX_ERR_ARG;
        }
        nb[k] = box_hi[k] - box_lo[k];
    }
    if (!free_is_box) return IGX_OK;
    long long I = 0;
    int i[3] = {0, 0, 0};
    for (i[0] = 0; i[0] < N[0]; ++i[0])
        for (i[1] = 0; i[1] < (d > 1 ? N[1] : 1); ++i[1])
            for (i[2] = 0; i[2] < (d > 2 ? N[2] : 1); ++i[2], ++I) {
                bool in = true;
                for (int k = 0; k < d; ++k) in = in && i[k] >= box_lo[k] && i[k] < box_hi[k];
                if (in != (s->h_free[base + I] != 0)) {
                    set_error("%s: the free dofs are not the box given (dof %lld)", what, base + I);
                    return IGX_ERR_ARG;
                }
            }
    return IGX_OK;
}

// the inverse on the box of nb dofs from box_lo on of the component at `base`, in the full-length vectors: (x) U_k^T reads the box
// of r, (x) U_k writes it into z
FastDiag box_fastdiag(const igx_solver *s, long long base, const int32_t *box_lo, const int *nb, const double *d_fac, int lam_mode,
                      long long batch, const int *dims)
{
    long long full_stride[4], off = base;
    box_strides(s->dim, dims ? dims : s->N, full_stride);
    for (int k = 0; k < s->dim; ++k) off += box_lo[k] * full_stride[k];
    return make_fastdiag(s->dim, nb, d_fac, full_stride, off, lam_mode, batch);
}

// The Kronecker inverse on the free box of the component at `base` of a patch solver, for the entry point `what`: checks the
// arguments, packs the factors and puts them on the device at d_fac in place of the previous ones (synchronised before and
// after).  *reset (or null) becomes IGX_PRECOND_NONE before anything is freed, whatever fails later.  nb out
int box_fastdiag_setup(igx_solver *s, long long base, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                       const double *const *lam, int lam_mode, const char *what, int *reset, double *&d_fac, int nb[3], const int *dims,
                       bool free_is_box)
{
    if (!box_lo || !box_hi || !U || !lam) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (lam_mode != IGX_KRON_SUM && lam_mode != IGX_KRON_PRODUCT) { set_error("%s: unknown lam_mode %d", what, lam_mode); return IGX_ERR_ARG; }
    nb[0] = nb[1] = nb[2] = 1;
    if (int rc = check_free_box(s, base, box_lo, box_hi, U, lam, nb, what, dims ? dims : s->N, free_is_box)) return rc;
    std::vector<double> h;
    pack_fastdiag(h, s->dim, nb, U, lam);
    if (reset) *reset = IGX_PRECOND_NONE;
    IGX_HIP(hipStreamSynchronize(s->ctx->stream));
    if (int rc = upload_replacing(s->ctx->stream, h, d_fac)) return rc;
    IGX_HIP(hipStreamSynchronize(s->ctx->stream));       // (h goes away)
    return IGX_OK;
}

// what multigrid.hip sees of a solver (mg_internal.h)
SolverRef solver_ref(const igx_solver *s)
{
    SolverRef R{s->ctx, s->mp, s->n, s->gw, s->d_mask, s->h_free.data(), s->precond, s->method, s->ncomp, s->n / s->ncomp, {}, s->symmetric};
    if (s->mp && s->ncomp > 1)
        for (int k = 0; k < s->ncomp * s->ncomp; ++k) R.blk[k] = s->block.blk[k];
    return R;
}

int refuse_multipatch_block(const igx_solver *s, const char *what)
{
    if (s && s->saddle) return refuse_saddle(s, what);           // (what a multipatch block solver does not serve, a saddle solver does not either)
    if (!s || !s->mp || s->ncomp < 2) return IGX_OK;
    set_error("%s: a multipatch block solver (igx_solver_create_multipatch_block) serves the linear solves, the SpMV and its "
              "Jacobi, Schwarz and multigrid (igx_solver_set_block_mg_*) preconditioners only", what);
    return IGX_ERR_UNSUPPORTED;
}

MgLevel *&solver_mg(igx_solver *s) { return s->mg; }

void solver_drop_mg_precond(igx_solver *s)
{
    if (s->precond == IGX_PRECOND_MG) s->precond = IGX_PRECOND_NONE;
}

int solver_check_sums(const igx_solver *s, const char *what)
{
    if (!s->mp) { set_error("%s: a multigrid level needs a multipatch solver", what); return IGX_ERR_UNSUPPORTED; }
    if (s->ncomp > 1) {                       // (a block solver owns its blocks: the sums may restart, the diagonal blocks must be there)
        for (int c = 0; c < s->ncomp; ++c)
            if (!s->block.blk[c * s->ncomp + c]) {
                set_error("%s: diagonal block (%d, %d) of a level of the multigrid hierarchy is missing (igx_solver_take_multipatch_block)",
                          what, c, c);
                return IGX_ERR_ARG;
            }
        return IGX_OK;
    }
    if (s->mp->generation != s->gen) {
        set_error("%s: the sums of a multipatch of the multigrid hierarchy were restarted (igx_multipatch_zero) since its solver was "
                  "made: make the solvers again", what);
        return IGX_ERR_ARG;
    }
    return IGX_OK;
}

int solver_residual(hipStream_t st, const igx_solver *s, const double *x, const double *b, double *y)
{
    return spmv(st, s, x, b, -1.0, y, nullptr, nullptr);
}

} // namespace igx

extern "C" {

int igx_solver_create(igx_patch *pt, int kind, const int64_t *fixed, int64_t nfixed, igx_solver **out)
{
    if (!create_args_ok(pt, fixed, nfixed, out, "igx_solver_create")) return IGX_ERR_ARG;
    if (!spd_kind(kind)) {
        set_error("igx_solver_create: CG needs a symmetric positive definite matrix (IGX_MASS or IGX_STIFFNESS), kind %d", kind);
        return IGX_ERR_UNSUPPORTED;
    }
    return create_patch_solver(pt, kind, 1, true, fixed, nfixed, out, "igx_solver_create");
}

int igx_solver_create_general(igx_patch *pt, int kind, const int64_t *fixed, int64_t nfixed, igx_solver **out)
{
    if (!create_args_ok(pt, fixed, nfixed, out, "igx_solver_create_general")) return IGX_ERR_ARG;
    if (kind != IGX_MASS && kind != IGX_STIFFNESS && kind != IGX_CONVDIFF && kind != IGX_FORM) {
        set_error("igx_solver_create_general: unknown kind %d", kind);
        return IGX_ERR_ARG;
    }
    igx_solver *s = nullptr;
    if (int rc = create_patch_solver(pt, kind, 1, true, fixed, nfixed, &s, "igx_solver_create_general")) return rc;
    if (int rc = init_bicgstab(s, "igx_solver_create_general")) { free_solver(s); return rc; }
    s->method = IGX_METHOD_BICGSTAB;
    *out = s;
    return IGX_OK;
}

int igx_solver_set_method(igx_solver *s, int method)
{
    if (!s) { set_error("igx_solver_set_method: null solver"); return IGX_ERR_ARG; }
    const bool known = method == IGX_METHOD_CG || method == IGX_METHOD_BICGSTAB || method == IGX_METHOD_MINRES;
    if (known && s->saddle != (method == IGX_METHOD_MINRES)) {
        set_error("igx_solver_set_method: MINRES is the method of saddle-point solvers (igx_solver_create_saddle), and their only one: "
                  "the matrix [[A, B^T], [B, 0]] is symmetric indefinite");
        return IGX_ERR_UNSUPPORTED;
    }
    if (method == IGX_METHOD_MINRES) return IGX_OK;
    if (method == IGX_METHOD_CG) {
        if (s->ncomp > 1 && !s->symmetric) {
            set_error("igx_solver_set_method: CG needs a symmetric positive definite matrix; the block solver was made as non-symmetric");
            return IGX_ERR_UNSUPPORTED;
        }
        if (s->parabolic && !s->symmetric) {
            set_error("igx_solver_set_method: CG needs a symmetric positive definite matrix; the parabolic solver was made as non-symmetric");
            return IGX_ERR_UNSUPPORTED;
        }
        if (s->ncomp == 1 && !s->mp && !s->parabolic && !spd_kind(s->kind) && !s->symmetric) {     // (symmetric: igx_solver_declare_symmetric)
            set_error("igx_solver_set_method: CG needs a symmetric positive definite matrix; kind %d is not known to be one", s->kind);
            return IGX_ERR_UNSUPPORTED;
        }
        s->method = method;
        return IGX_OK;
    }
    if (method != IGX_METHOD_BICGSTAB) { set_error("igx_solver_set_method: unknown method %d", method); return IGX_ERR_ARG; }
    if (s->precond == IGX_PRECOND_MG) {
        set_error("igx_solver_set_method: the multigrid preconditioner serves CG only: select another preconditioner first");
        return IGX_ERR_UNSUPPORTED;
    }
    IGX_HIP(hipSetDevice(s->ctx->device));
    if (int rc = init_bicgstab(s, "igx_solver_set_method")) return rc;
    s->method = method;
    return IGX_OK;
}

int igx_solver_last_breakdown(const igx_solver *s) { return !s ? 0 : s->saddle ? s->sad.breakdown : s->bicg.breakdown; }

int igx_solver_create_multipatch(igx_multipatch *mp, const int64_t *fixed, int64_t nfixed, igx_solver **out)
{
    if (!create_args_ok(mp, fixed, nfixed, out, "igx_solver_create_multipatch")) return IGX_ERR_ARG;
    if (hipSetDevice(mp->ctx->device) != hipSuccess) { set_error("igx_solver_create_multipatch: hipSetDevice failed"); return IGX_ERR_HIP; }
    igx_solver *s = new igx_solver;
    s->ctx = mp->ctx; s->mp = mp; s->gen = mp->generation; s->kind = -1; s->n = mp->nglobal;
    if (int rc = init_solver(s, fixed, nfixed, mp->max_row, {}, "igx_solver_create_multipatch")) return rc;
    *out = s;
    return IGX_OK;
}

int igx_solver_create_multipatch_block(igx_multipatch *mp, int ncomp, int symmetric, const int64_t *fixed, int64_t nfixed, igx_solver **out)
{
    const char *what = "igx_solver_create_multipatch_block";
    if (!create_args_ok(mp, fixed, nfixed, out, what)) return IGX_ERR_ARG;
    if (ncomp != 2 && ncomp != 3) { set_error("%s: ncomp must be 2 or 3, not %d", what, ncomp); return IGX_ERR_ARG; }
    if (hipSetDevice(mp->ctx->device) != hipSuccess) { set_error("%s: hipSetDevice failed", what); return IGX_ERR_HIP; }
    igx_solver *s = new igx_solver;
    // (the blocks are the solver's own copies: it is not bound to the generation of the multipatch's sums)
    s->ctx = mp->ctx; s->mp = mp; s->gen = mp->generation; s->kind = -1; s->ncomp = ncomp; s->n = ncomp * mp->nglobal;
    s->symmetric = symmetric != 0;
    if (int rc = init_solver(s, fixed, nfixed, mp->max_row, {}, what)) return rc;
    if (!s->symmetric) {
        if (int rc = init_bicgstab(s, what)) { free_solver(s); return rc; }
        s->method = IGX_METHOD_BICGSTAB;
    }
    *out = s;
    return IGX_OK;
}

int igx_solver_take_multipatch_block(igx_solver *s, int p, int q)
{
    const char *what = "igx_solver_take_multipatch_block";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->mp || s->ncomp < 2) { set_error("%s: not a multipatch block solver (igx_solver_create_multipatch_block)", what); return IGX_ERR_ARG; }
    if (p < 0 || p >= s->ncomp || q < 0 || q >= s->ncomp) { set_error("%s: block (%d, %d) of %d components", what, p, q, s->ncomp); return IGX_ERR_ARG; }
    double *&dst = s->block.blk[p * s->ncomp + q];
    if (dst) { set_error("%s: block (%d, %d) was taken already", what, p, q); return IGX_ERR_ARG; }
    const igx_multipatch *mp = s->mp;
    if (mp->scattered != mp->generation) {
        set_error("%s: nothing was scattered into the multipatch's sums since they were restarted (igx_multipatch_zero clears the "
                  "interface rows only): scatter every patch first", what);
        return IGX_ERR_ARG;
    }
    IGX_HIP(hipSetDevice(s->ctx->device));
    double *copy = nullptr;
    if (hipMalloc((void **)&copy, (size_t)mp->nnz * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: out of device memory (%.3f GB)", what, 8.0 * mp->nnz / 1e9);
        return IGX_ERR_NOMEM;
    }
    if (int rc = igx_multipatch_values_d(mp, copy)) { (void)hipFree(copy); return rc; }
    dst = copy;
    return IGX_OK;
}

int igx_solver_download_multipatch_block(const igx_solver *s, int p, int q, double *vals)
{
    const char *what = "igx_solver_download_multipatch_block";
    if (!s || !vals) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->mp || s->ncomp < 2) { set_error("%s: not a multipatch block solver (igx_solver_create_multipatch_block)", what); return IGX_ERR_ARG; }
    if (p < 0 || p >= s->ncomp || q < 0 || q >= s->ncomp) { set_error("%s: block (%d, %d) of %d components", what, p, q, s->ncomp); return IGX_ERR_ARG; }
    const double *src = s->block.blk[p * s->ncomp + q];
    if (!src) { set_error("%s: block (%d, %d) is absent", what, p, q); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipMemcpyAsync(vals, src, (size_t)s->mp->nnz * sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_solver_create_block(igx_patch *pt, int ncomp, int symmetric, const int64_t *fixed, int64_t nfixed, igx_solver **out)
{
    const char *what = "igx_solver_create_block";
    if (!create_args_ok(pt, fixed, nfixed, out, what)) return IGX_ERR_ARG;
    if (ncomp != 2 && ncomp != 3) { set_error("%s: ncomp must be 2 or 3, not %d", what, ncomp); return IGX_ERR_ARG; }
    igx_solver *s = nullptr;
    if (int rc = create_patch_solver(pt, IGX_FORM, ncomp, false, fixed, nfixed, &s, what)) return rc;
    s->symmetric = symmetric != 0;
    if (!s->symmetric) {
        if (int rc = init_bicgstab(s, what)) { free_solver(s); return rc; }
        s->method = IGX_METHOD_BICGSTAB;
    }
    *out = s;
    return IGX_OK;
}

int igx_solver_take_block(igx_solver *s, int p, int q)
{
    const char *what = "igx_solver_take_block";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (s->ncomp < 2 || s->mp) { set_error("%s: not a block solver of a patch (igx_solver_create_block)", what); return IGX_ERR_ARG; }
    if (p < 0 || p >= s->ncomp || q < 0 || q >= s->ncomp) { set_error("%s: block (%d, %d) of %d components", what, p, q, s->ncomp); return IGX_ERR_ARG; }
    double *&dst = s->block.blk[p * s->ncomp + q];
    if (dst) { set_error("%s: block (%d, %d) was taken already", what, p, q); return IGX_ERR_ARG; }
    igx_patch *pt = s->pt;
    if (pt->values_kind != IGX_FORM || !pt->d_data) {
        set_error("%s: the patch holds no IGX_FORM values: assemble them first (igx_assemble, data_out may be NULL)", what);
        return IGX_ERR_ARG;
    }
    IGX_HIP(hipSetDevice(s->ctx->device));
    IGX_HIP(hipStreamSynchronize(pt->ctx->stream));
    dst = pt->d_data;                               // the buffer changes hands: the patch's next assembly allocates anew
    pt->d_data = nullptr;
    pt->values_kind = -1;
    return IGX_OK;
}

int igx_solver_replace_block(igx_solver *s, int p, int q)
{
    const char *what = "igx_solver_replace_block";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (s->ncomp < 2 || s->mp) { set_error("%s: not a block solver of a patch (igx_solver_create_block)", what); return IGX_ERR_ARG; }
    if (p < 0 || p >= s->ncomp || q < 0 || q >= s->ncomp) { set_error("%s: block (%d, %d) of %d components", what, p, q, s->ncomp); return IGX_ERR_ARG; }
    if (s->eig) { set_error("%s: the solver holds an eigen-solver session, whose pieces were made for the present blocks", what); return IGX_ERR_UNSUPPORTED; }
    igx_patch *pt = s->pt;
    if (pt->values_kind != IGX_FORM || !pt->d_data) {
        set_error("%s: the patch holds no IGX_FORM values: assemble them first (igx_assemble, data_out may be NULL)", what);
        return IGX_ERR_ARG;
    }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipStreamSynchronize(pt->ctx->stream));
    IGX_HIP(hipStreamSynchronize(st));              // (no product of the solver reads the old values any more)
    double *&dst = s->block.blk[p * s->ncomp + q];
    double *old = dst;
    dst = pt->d_data;                               // the buffers change hands: the old block is the patch's next values buffer
    pt->d_data = old;                               // (both were allocated by igx_assemble for this patch: one size), or none yet
    pt->values_kind = -1;
    s->block.hidden[p * s->ncomp + q] = false;
    if (p == q && s->precond == IGX_PRECOND_JACOBI) {
        const long long N = s->saddle ? s->sad.nu : s->n / s->ncomp;
        jacobi_diagonal(st, s, dst, s->dinv + p * N, p);
        IGX_HIP(hipGetLastError());
        IGX_HIP(hipStreamSynchronize(st));
    }
    return IGX_OK;
}

int igx_solver_hide_block(igx_solver *s, int p, int q, int hidden)
{
    const char *what = "igx_solver_hide_block";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->saddle) { set_error("%s: saddle-point solvers only (igx_solver_create_saddle)", what); return IGX_ERR_UNSUPPORTED; }
    if (p < 0 || p >= s->ncomp || q < 0 || q >= s->ncomp || p == q) { set_error("%s: (%d, %d) is not an off-diagonal block of %d components", what, p, q, s->ncomp); return IGX_ERR_ARG; }
    s->block.hidden[p * s->ncomp + q] = hidden != 0;      // (read on the host at every launch: the next product sees it)
    return IGX_OK;
}

int igx_solver_set_block_kron(igx_solver *s, int comp, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                              const double *const *lam, int mode)
{
    const char *what = "igx_solver_set_block_kron";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->saddle)                                 // (a saddle solver: the velocity part of its block-diagonal preconditioner)
        if (int rc = refuse_multipatch_block(s, what)) return rc;
    if (s->ncomp < 2) { set_error("%s: not a block solver (igx_solver_create_block)", what); return IGX_ERR_ARG; }
    if (comp < 0 || comp >= s->ncomp) { set_error("%s: component %d of %d", what, comp, s->ncomp); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    const long long base = (long long)comp * s->g.nrows;
    int nb[3];
    // (a Kronecker preconditioner in use is dropped: selected again by igx_solver_set_precond)
    if (int rc = box_fastdiag_setup(s, base, box_lo, box_hi, U, lam, mode, what, s->precond == IGX_PRECOND_KRON ? &s->precond : nullptr,
                                    s->block.d_bkron[comp], nb)) return rc;
    const long long nbox = (long long)nb[0] * nb[1] * nb[2];
    if (nbox > s->wlen)                            // the two work buffers fit the largest box of any component
        if (int rc = alloc_fastdiag_work(s, nbox)) return rc;
    s->block.bkron[comp] = box_fastdiag(s, base, box_lo, nb, s->block.d_bkron[comp], mode);
    for (int k = 0; k < 3; ++k) { s->block.klo[comp][k] = k < s->dim ? box_lo[k] : 0; s->block.knb[comp][k] = nb[k]; }
    s->block.kmode[comp] = mode;
    if (s->eig) eig_drop_block_kron(s);            // (the eigen pieces sized their work buffers for the previous boxes)
    return IGX_OK;
}

int igx_solver_take_mass(igx_solver *s)
{
    const char *what = "igx_solver_take_mass";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (int rc = refuse_multipatch_block(s, what)) return rc;
    if (s->ncomp < 2) { set_error("%s: not a block solver (igx_solver_create_block)", what); return IGX_ERR_ARG; }
    if (s->block.mass) { set_error("%s: the mass matrix was taken already", what); return IGX_ERR_ARG; }
    igx_patch *pt = s->pt;
    if ((pt->values_kind != IGX_MASS && pt->values_kind != IGX_FORM) || !pt->d_data) {
        set_error("%s: the patch holds no IGX_MASS or IGX_FORM values: assemble them first (igx_assemble, data_out may be NULL)", what);
        return IGX_ERR_ARG;
    }
    IGX_HIP(hipSetDevice(s->ctx->device));
    IGX_HIP(hipStreamSynchronize(pt->ctx->stream));
    s->block.mass = pt->d_data;                     // the buffer changes hands, as a block does
    pt->d_data = nullptr;
    pt->values_kind = -1;
    return IGX_OK;
}

void igx_solver_destroy(igx_solver *s)
{
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    free_solver(s);
}

int igx_solver_set_precond(igx_solver *s, int precond, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                           const double *const *lam, int lam_mode)
{
    if (!s) { set_error("igx_solver_set_precond: null solver"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    s->step.step_precond = -1;                                // (a stepping session's preconditioner data is replaced: set it again)
    s->step.pc_vals = -1;
    if (s->saddle) return saddle_set_precond(s, precond);
    if (precond == IGX_PRECOND_NONE) { s->precond = precond; return IGX_OK; }
    if (precond == IGX_PRECOND_JACOBI) {
        if (int rc = check_values(s, "igx_solver_set_precond")) return rc;
        if (s->ncomp > 1) {                                   // component c: the diagonal of block (c, c) at offset c (scalar rows)
            const long long N = s->n / s->ncomp;
            for (int c = 0; c < s->ncomp; ++c) jacobi_diagonal(st, s, s->block.blk[c * s->ncomp + c], s->dinv + c * N, c);
        } else if (s->mp) jacobi_diagonal(st, s, s->mp->d_vals, s->dinv);
        else jacobi_diagonal(st, s, patch_values(s), s->dinv);
        IGX_HIP(hipGetLastError());
        IGX_HIP(hipStreamSynchronize(st));
        s->precond = precond;
        return IGX_OK;
    }
    if (precond == IGX_PRECOND_SCHWARZ) {
        if (!s->mp) { set_error("igx_solver_set_precond: the Schwarz preconditioner needs a multipatch solver"); return IGX_ERR_UNSUPPORTED; }
        if (s->ncomp > 1) {                                   // the factors of every component, set by igx_solver_set_block_schwarz
            for (int c = 0; c < s->ncomp; ++c)
                if (s->block.bsw[c].empty()) {
                    set_error("igx_solver_set_precond: set the Schwarz factors of component %d first (igx_solver_set_block_schwarz)", c);
                    return IGX_ERR_ARG;
                }
            s->precond = precond;
            return IGX_OK;
        }
        if (s->sw.empty() || !s->d_W) { set_error("igx_solver_set_precond: set the Schwarz factors up first (igx_solver_set_schwarz)"); return IGX_ERR_ARG; }
        s->precond = precond;
        return IGX_OK;
    }
    if (precond == IGX_PRECOND_MG && s->mp && s->ncomp > 1) {    // the hierarchy of igx_solver_set_block_mg_*, once it is complete
        if (!s->symmetric || s->method != IGX_METHOD_CG) {
            set_error("igx_solver_set_precond: the multigrid preconditioner serves CG on a block solver made as symmetric only");
            return IGX_ERR_UNSUPPORTED;
        }
        if (mg_check(s, "igx_solver_set_precond(IGX_PRECOND_MG)")) return IGX_ERR_UNSUPPORTED;     // (mg_check's message stands)
        s->precond = precond;
        return IGX_OK;
    }
    if (precond == IGX_PRECOND_MG) {
        if (!s->mp) { set_error("igx_solver_set_precond: the multigrid preconditioner needs a multipatch solver"); return IGX_ERR_UNSUPPORTED; }
        if (s->method != IGX_METHOD_CG) { set_error("igx_solver_set_precond: the multigrid preconditioner serves CG only"); return IGX_ERR_UNSUPPORTED; }
        if (int rc = mg_check(s, "igx_solver_set_precond")) return rc;
        s->precond = precond;
        return IGX_OK;
    }
    if (precond != IGX_PRECOND_KRON) { set_error("igx_solver_set_precond: unknown preconditioner %d", precond); return IGX_ERR_ARG; }
    if (s->mp) { set_error("igx_solver_set_precond: IGX_PRECOND_KRON needs a patch solver (multipatch: IGX_PRECOND_SCHWARZ)"); return IGX_ERR_UNSUPPORTED; }
    if (s->ncomp > 1) {                                   // the factors of every component, set by igx_solver_set_block_kron
        for (int c = 0; c < s->ncomp; ++c)
            if (!s->block.d_bkron[c]) {
                set_error("igx_solver_set_precond: set the Kronecker factors of component %d first (igx_solver_set_block_kron)", c);
                return IGX_ERR_ARG;
            }
        s->precond = precond;
        return IGX_OK;
    }
    int nb[3];
    if (int rc = box_fastdiag_setup(s, 0, box_lo, box_hi, U, lam, lam_mode, "igx_solver_set_precond", &s->precond, s->d_kron, nb)) return rc;
    if (int rc = alloc_fastdiag_work(s, (long long)nb[0] * nb[1] * nb[2])) return rc;
    s->kron = box_fastdiag(s, 0, box_lo, nb, s->d_kron, lam_mode);
    s->precond = IGX_PRECOND_KRON;
    return IGX_OK;
}

// The host side of a Schwarz set-up over the multipatch of s (igx_solver_set_schwarz; igx_solver_set_block_schwarz per component):
// the arguments checked, then per patch with a non-empty box its map in sw and, per axis, U_k^T | U_k | lam_k at fac[j] in h;
// wlen: the largest box
static int pack_schwarz(const igx_solver *s, const int32_t *box_lo, const int32_t *box_hi, const double *const *U, const double *const *lam,
                        int lam_mode, const char *what, std::vector<SwPatch> &sw, std::vector<size_t> &fac, std::vector<double> &h,
                        long long &wlen)
{
    if (!s->mp) { set_error("%s: the Schwarz preconditioner needs a multipatch solver", what); return IGX_ERR_UNSUPPORTED; }
    const igx_multipatch *mp = s->mp;
    if (!mp->injective) {
        set_error("%s: a local-to-global map is not injective (two dofs of one patch share a global dof); "
                  "use IGX_PRECOND_JACOBI", what);
        return IGX_ERR_UNSUPPORTED;
    }
    if (!box_lo || !box_hi || !U || !lam) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (lam_mode != IGX_KRON_SUM && lam_mode != IGX_KRON_PRODUCT) { set_error("%s: unknown lam_mode %d", what, lam_mode); return IGX_ERR_ARG; }
    wlen = 1;
    for (int p = 0; p < mp->np; ++p) {
        const auto &P = mp->pp[p];
        bool empty = false;
        for (int k = 0; k < P.dim; ++k) {
            const int lo = box_lo[p * 3 + k], hi = box_hi[p * 3 + k];
            if (lo < 0 || hi > P.N[k] || lo > hi) {
                set_error("%s: patch %d: bad box [%d, %d) on axis %d of %d dofs", what, p, lo, hi, k, P.N[k]);
                return IGX_ERR_ARG;
            }
            empty = empty || lo == hi;
        }
        if (empty) continue;
        SwPatch W{};
        const int off = 3 - P.dim;
        for (int a = 0; a < 3; ++a) { W.map.lo[a] = 0; W.map.nb[a] = 1; W.map.N[a] = 1; }
        W.map.nbox = 1;
        for (int k = 0; k < P.dim; ++k) {
            const int m = box_hi[p * 3 + k] - box_lo[p * 3 + k];
            if (!U[p * 3 + k] || !lam[p * 3 + k]) { set_error("%s: patch %d: factor of axis %d missing", what, p, k); return IGX_ERR_ARG; }
            W.map.lo[off + k] = box_lo[p * 3 + k]; W.map.nb[off + k] = m; W.map.N[off + k] = P.N[k];
            W.map.nbox *= m;
        }
        W.map.l2g = P.d_l2g;
        W.F.dim = P.dim;
        fac.push_back(pack_fastdiag(h, P.dim, W.map.nb + off, U + p * 3, lam + p * 3));
        wlen = std::max(wlen, W.map.nbox);
        sw.push_back(W);
    }
    if (sw.empty()) { set_error("%s: every patch box is empty", what); return IGX_ERR_ARG; }
    return IGX_OK;
}

// the fast-diagonalization plans of the packed patches over their factors on the device (compact box vectors in and out)
static void plan_schwarz(std::vector<SwPatch> &sw, const std::vector<size_t> &fac, const double *d_fac, int lam_mode)
{
    for (size_t j = 0; j < sw.size(); ++j) {
        const int d = sw[j].F.dim;
        const int *m = sw[j].map.nb + (3 - d);
        long long stride[4];
        box_strides(d, m, stride);
        sw[j].F = make_fastdiag(d, m, d_fac + fac[j], stride, 0, lam_mode);
    }
}

int igx_solver_set_schwarz(igx_solver *s, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                           const double *const *lam, int lam_mode)
{
    const char *what = "igx_solver_set_schwarz";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (s->mp && s->ncomp > 1) {
        set_error("%s: a multipatch block solver takes its Schwarz factors per component (igx_solver_set_block_schwarz)", what);
        return IGX_ERR_UNSUPPORTED;
    }
    std::vector<SwPatch> sw;
    std::vector<size_t> fac;
    std::vector<double> h;
    long long wlen = 1;
    if (int rc = pack_schwarz(s, box_lo, box_hi, U, lam, lam_mode, what, sw, fac, h, wlen)) return rc;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipStreamSynchronize(st));
    (void)hipFree(s->d_box); s->d_box = nullptr;
    s->sw.clear();
    if (s->precond == IGX_PRECOND_SCHWARZ) s->precond = IGX_PRECOND_NONE;
    if (int rc = upload_replacing(st, h, s->d_kron)) return rc;
    if (int rc = alloc_fastdiag_work(s, wlen)) return rc;
    IGX_HIP(hipMalloc((void **)&s->d_box, (size_t)wlen * sizeof(double)));
    plan_schwarz(sw, fac, s->d_kron, lam_mode);
    IGX_HIP(hipStreamSynchronize(st));
    s->sw = std::move(sw);
    s->precond = IGX_PRECOND_SCHWARZ;
    return IGX_OK;
}

int igx_solver_set_block_schwarz(igx_solver *s, int comp, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                                 const double *const *lam, int lam_mode)
{
    const char *what = "igx_solver_set_block_schwarz";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->mp || s->ncomp < 2) { set_error("%s: not a multipatch block solver (igx_solver_create_multipatch_block)", what); return IGX_ERR_ARG; }
    if (comp < 0 || comp >= s->ncomp) { set_error("%s: component %d of %d", what, comp, s->ncomp); return IGX_ERR_ARG; }
    std::vector<SwPatch> sw;
    std::vector<size_t> fac;
    std::vector<double> h;
    long long wlen = 1;
    if (int rc = pack_schwarz(s, box_lo, box_hi, U, lam, lam_mode, what, sw, fac, h, wlen)) return rc;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipStreamSynchronize(st));
    // (a Schwarz preconditioner in use is dropped: selected again by igx_solver_set_precond once every component is set)
    if (s->precond == IGX_PRECOND_SCHWARZ) s->precond = IGX_PRECOND_NONE;
    s->block.bsw[comp].clear();
    if (int rc = upload_replacing(st, h, s->block.d_bkron[comp])) return rc;
    if (wlen > s->wlen || !s->d_box) {                 // the work buffers and the box fit the largest box of any component
        wlen = std::max(wlen, s->wlen);
        (void)hipFree(s->d_box); s->d_box = nullptr;
        if (int rc = alloc_fastdiag_work(s, wlen)) return rc;
        IGX_HIP(hipMalloc((void **)&s->d_box, (size_t)wlen * sizeof(double)));
    }
    plan_schwarz(sw, fac, s->block.d_bkron[comp], lam_mode);
    IGX_HIP(hipStreamSynchronize(st));                  // (h goes away)
    s->block.bsw[comp] = std::move(sw);
    return IGX_OK;
}

int igx_solver_precond_d(igx_solver *s, const double *d_r, double *d_z)
{
    if (!s || !d_r || !d_z) { set_error("igx_solver_precond_d: null argument"); return IGX_ERR_ARG; }
    if (d_r == d_z) { set_error("igx_solver_precond_d: d_r and d_z must be different buffers (z is cleared before r is read)"); return IGX_ERR_ARG; }
    if (int rc = check_values(s, "igx_solver_precond_d")) return rc;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const unsigned nb = (unsigned)((s->n + 255) / 256);
    if (s->saddle) {                                       // (the masked r in s->w: the pressure inverse reads fixed dofs as 0)
        mask_copy(st, s, d_r, s->w);
        if (int rc = saddle_apply_precond(st, s, s->w, d_z)) return rc;
        IGX_HIP(hipGetLastError());
        IGX_HIP(hipStreamSynchronize(st));
        return IGX_OK;
    }
    switch (s->precond) {
    case IGX_PRECOND_JACOBI: k_scale<<<nb, 256, 0, st>>>(s->n, s->dinv, d_r, d_z); break;
    case IGX_PRECOND_KRON:
        IGX_HIP(hipMemsetAsync(d_z, 0, (size_t)s->n * sizeof(double), st));
        if (int rc = apply_kron(st, s, d_r, d_z)) return rc;
        break;
    case IGX_PRECOND_SCHWARZ:
        if (int rc = apply_schwarz(st, s, d_r, d_z)) return rc;
        break;
    case IGX_PRECOND_MG:                                   // (the V-cycle reads r with zeros on the fixed dofs)
        mask_copy(st, s, d_r, s->w);
        if (int rc = mg_apply(st, s, s->w, d_z)) return rc;
        break;
    default: mask_copy(st, s, d_r, d_z); break;
    }
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_solver_spmv_d(igx_solver *s, const double *d_x, double *d_y)
{
    if (!s || !d_x || !d_y) { set_error("igx_solver_spmv_d: null argument"); return IGX_ERR_ARG; }
    if (int rc = check_values(s, "igx_solver_spmv_d")) return rc;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    mask_copy(st, s, d_x, s->w);
    IGX_HIP(hipGetLastError());
    if (int rc = spmv(st, s, s->w, nullptr, 1.0, d_y, nullptr, nullptr)) return rc;
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

} // extern "C"

namespace igx {

// the end of a call between the events `begin` and `end`: the stream drained, a kernel failure reported under `what`, the time out
int close_call(hipStream_t st, hipEvent_t begin, hipEvent_t end, const char *what, float &total_ms)
{
    IGX_HIP(hipEventRecord(end, st));
    IGX_HIP(hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: kernel failure: %s", what, hipGetErrorString(e)); return IGX_ERR_HIP; }
    (void)hipEventElapsedTime(&total_ms, begin, end);
    return IGX_OK;
}

// the solution x + ext(g) to the host, the device time of the whole solve (from ev[5]) and the info block
static int finish_solve(hipStream_t st, igx_solver *s, const double *gvals, double *u, igx_solve_info *info, igx_solve_info &inf)
{
    IGX_HIP(hipMemcpyAsync(u, s->x, (size_t)s->n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (int rc = close_call(st, s->ev[5], s->ev[4], "igx_solver_solve", inf.total_ms)) return rc;
    for (size_t k = 0; k < s->fixed.size(); ++k) u[s->fixed[k]] = gvals[k];
    inf.n_free = s->n - (long long)s->fixed.size();
    if (info) *info = inf;
    return IGX_OK;
}

// The device entry of the solves: R A R^T x = R (b - A w) with b in s->b and w = ext(g) in s->w (both on the device, full
// length).  With x0_in_x the initial guess is in s->x already, zero on the fixed dofs; else x starts at 0.  r = R (b - A w), its
// norm the reference of the relative residual; r -= A x0; then CG or BiCGStab (s->method).  The free part of the solution stays
// in s->x (zero on the fixed dofs).  `lift`: the vector w (s->w, or another full-length device vector), or null: nothing is
// lifted, r = R b (the stages of a Rosenbrock method, whose unknowns vanish on the fixed dofs).  The matrix is the one spmv()
// multiplies by (a parabolic solver: C, or the values of s->par.vals_sel) and the preconditioner the one s holds now.
// `from_guess` (with x0_in_x): the stop is relative to the residual the initial guess leaves, ||r|| <= tol ||r0||, as the
// reference's Newton measures it (pyiga/solvers.py:350-354: rtol times the residual at the start value): the solve is then one
// for the increment x - x0, and its tolerance refers to the change of a stage and not to the 1/(tau |F|) times larger state.  A
// guess that meets tol ||R (b - A w)|| already is the solution (no iteration), and the stop is never below
// 100 eps ||R (b - A w)||, which the true residual cannot be seen to pass.
int solve_lifted(hipStream_t st, igx_solver *s, const double *lift, bool x0_in_x, double tol, int maxiter, int check_every, int timed,
                 igx_solve_info &inf, bool from_guess)
{
    if (s->saddle) return saddle_solve_lifted(st, s, lift, x0_in_x, tol, maxiter, check_every, timed, inf);
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    if (!x0_in_x) IGX_HIP(hipMemsetAsync(s->x, 0, nbytes, st));
    IGX_HIP(hipMemsetAsync(s->p, 0, nbytes, st));
    IGX_HIP(hipMemsetAsync(s->q, 0, nbytes, st));
    IGX_HIP(hipMemsetAsync(s->z, 0, nbytes, st));
    IGX_HIP(hipMemsetAsync(s->d_sc, 0, SC_N * sizeof(double), st));
    const unsigned nbv = vec_blocks(n);
    double *pA = s->d_part;
    // r = R (b - A ext(g)); its norm is the reference of the relative residual
    if (lift) {
        if (int rc = spmv(st, s, lift, s->b, -1.0, s->r, nullptr, nullptr)) return rc;
    } else mask_copy(st, s, s->b, s->r);
    k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->r, s->r, nullptr, nullptr, pA, nullptr);
    k_fin<<<1, BLOCK, 0, st>>>(pA, nullptr, nbv, s->d_sc, FIN_INIT);
    double h_rr = 0.0;
    IGX_HIP(hipMemcpyAsync(&h_rr, s->d_sc + SC_RR, sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    double bnorm = std::sqrt(h_rr);
    if (x0_in_x) {
        if (int rc = spmv(st, s, s->x, s->r, -1.0, s->r, nullptr, nullptr)) return rc;
        if (from_guess) {
            k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->r, s->r, nullptr, nullptr, pA, nullptr);
            if (int rc = sum_partials(st, s, nbv, &h_rr)) return rc;
            IGX_HIP(hipMemsetAsync(s->d_sc, 0, SC_N * sizeof(double), st));
            // (not below what double precision resolves of the true residual: 100 eps ||R (b - A w)||)
            if (std::sqrt(h_rr) > tol * bnorm) bnorm = std::max(std::sqrt(h_rr), 100.0 * 2.220446049250313e-16 * bnorm / tol);
        }
    }
    return s->method == IGX_METHOD_BICGSTAB ? solve_bicgstab(st, s, bnorm, tol, maxiter, check_every, timed, inf)
                                            : solve_cg(st, s, bnorm, tol, maxiter, check_every, timed, inf);
}

} // namespace igx

extern "C" {

int igx_solver_solve(igx_solver *s, const double *b, const double *gvals, const double *x0, double tol, int maxiter, int check_every,
                     int timed, double *u, igx_solve_info *info)
{
    // (b may be null on a scalar multipatch solver only: the multipatch's summed vector has scalar length)
    if (!s || (!b && (!s->mp || s->ncomp > 1)) || (!gvals && !s->fixed.empty()) || !u) { set_error("igx_solver_solve: null argument"); return IGX_ERR_ARG; }
    if (!(tol >= 0.0) || maxiter < 0) { set_error("igx_solver_solve: tol must be >= 0 and maxiter >= 0"); return IGX_ERR_ARG; }
    if (int rc = check_values(s, "igx_solver_solve")) return rc;
    if (check_every < 1) check_every = 1;
    s->bicg.breakdown = 0;
    s->sad.breakdown = 0;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    igx_solve_info inf{};
    // ext(g) (+ the free part of x0): the vector the lifted right-hand side is formed with
    std::vector<double> w((size_t)n, 0.0);
    for (size_t k = 0; k < s->fixed.size(); ++k) w[s->fixed[k]] = gvals[k];
    IGX_HIP(hipEventRecord(s->ev[5], st));
    if (b) IGX_HIP(hipMemcpyAsync(s->b, b, nbytes, hipMemcpyHostToDevice, st));
    else IGX_HIP(hipMemcpyAsync(s->b, s->mp->d_vec, nbytes, hipMemcpyDeviceToDevice, st));      // the multipatch's summed vector
    IGX_HIP(hipMemcpyAsync(s->w, w.data(), nbytes, hipMemcpyHostToDevice, st));
    if (x0) {
        std::vector<double> xf((size_t)n);
        for (long long i = 0; i < n; ++i) xf[i] = s->h_free[i] ? x0[i] : 0.0;
        IGX_HIP(hipMemcpyAsync(s->x, xf.data(), nbytes, hipMemcpyHostToDevice, st));
        IGX_HIP(hipStreamSynchronize(st));                   // (xf leaves scope)
    }
    if (int rc = solve_lifted(st, s, s->w, x0 != nullptr, tol, maxiter, check_every, timed, inf)) return rc;
    return finish_solve(st, s, gvals, u, info, inf);
}

} // extern "C"

// --- Newton's method on a patch solver: the iterate, the residual and the Jacobian stay on the device ----
// x -= d (the Newton update; d vanishes on the fixed dofs)
__global__ void k_sub(long long n, double *x, const double *d)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] -= d[i];
}

extern "C" {

static int newton_solver_ok(const igx_solver *s, const char *what)
{
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (s->mp || s->ncomp > 1 || s->parabolic) { set_error("%s: scalar patch solvers only", what); return IGX_ERR_UNSUPPORTED; }
    return IGX_OK;
}

int igx_solver_declare_symmetric(igx_solver *s)
{
    if (int rc = newton_solver_ok(s, "igx_solver_declare_symmetric")) return rc;
    s->symmetric = true;
    return IGX_OK;
}

int igx_solver_values_changed(igx_solver *s)
{
    if (int rc = newton_solver_ok(s, "igx_solver_values_changed")) return rc;
    if (int rc = check_values(s, "igx_solver_values_changed")) return rc;
    if (s->precond != IGX_PRECOND_JACOBI) return IGX_OK;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    jacobi_diagonal(st, s, patch_values(s), s->dinv);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_solver_masked_norm_d(igx_solver *s, const double *d_v, double *norm)
{
    if (int rc = newton_solver_ok(s, "igx_solver_masked_norm_d")) return rc;
    if (!d_v || !norm) { set_error("igx_solver_masked_norm_d: null argument"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const long long n = s->n;
    const unsigned nbv = vec_blocks(n);
    IGX_HIP(hipMemsetAsync(s->d_sc, 0, SC_N * sizeof(double), st));
    mask_copy(st, s, d_v, s->r);
    k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->r, s->r, nullptr, nullptr, s->d_part, nullptr);
    double h_rr = 0.0;
    if (int rc = sum_partials(st, s, nbv, &h_rr)) return rc;
    *norm = std::sqrt(h_rr);
    return IGX_OK;
}

int igx_solver_newton_update_d(igx_solver *s, const double *d_F, double *d_x, double tol, int maxiter, int check_every, igx_solve_info *info)
{
    if (int rc = newton_solver_ok(s, "igx_solver_newton_update_d")) return rc;
    if (!d_F || !d_x) { set_error("igx_solver_newton_update_d: null argument"); return IGX_ERR_ARG; }
    if (!(tol >= 0.0) || maxiter < 0) { set_error("igx_solver_newton_update_d: tol must be >= 0 and maxiter >= 0"); return IGX_ERR_ARG; }
    if (int rc = check_values(s, "igx_solver_newton_update_d")) return rc;
    if (check_every < 1) check_every = 1;
    s->bicg.breakdown = 0;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const long long n = s->n;
    igx_solve_info inf{};
    IGX_HIP(hipEventRecord(s->ev[5], st));
    IGX_HIP(hipMemcpyAsync(s->b, d_F, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    // nothing is lifted: the increment vanishes on the fixed dofs, r = R F, the solve starts from zero
    if (int rc = solve_lifted(st, s, nullptr, false, tol, maxiter, check_every, 0, inf)) return rc;
    k_sub<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, d_x, s->x);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipEventRecord(s->ev[4], st));
    IGX_HIP(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&inf.total_ms, s->ev[5], s->ev[4]);
    inf.n_free = n - (long long)s->fixed.size();
    if (info) *info = inf;
    return IGX_OK;
}

int igx_kron_apply_d(igx_ctx *ctx, const igx_kron_desc *d, const double *d_x, double *d_y, double *d_work, int64_t work_len)
{
    if (!ctx || !d || !d_x || !d_y) { set_error("igx_kron_apply_d: null argument"); return IGX_ERR_ARG; }
    if (d->dim < 1 || d->dim > 3 || d->batch < 1) { set_error("igx_kron_apply_d: dim must be 1..3 and batch >= 1"); return IGX_ERR_ARG; }
    if (d->lam_mode < 0 || d->lam_mode > IGX_KRON_PRODUCT) { set_error("igx_kron_apply_d: unknown lam_mode %d", d->lam_mode); return IGX_ERR_ARG; }
    KronPlan P{};
    P.dim = d->dim;
    P.batch = d->batch;
    for (int k = 0; k < d->dim; ++k) {
        if (d->m[k] < 1 || d->n[k] < 1 || !d->d_B[k] || (d->lam_mode && !d->d_lam[k])) {
            set_error("igx_kron_apply_d: factor %d is empty or missing", k);
            return IGX_ERR_ARG;
        }
        P.m[k] = d->m[k]; P.n[k] = d->n[k]; P.B[k] = d->d_B[k]; P.lam[k] = d->d_lam[k];
    }
    for (int k = 0; k < 4; ++k) { P.x_stride[k] = d->x_stride[k]; P.y_stride[k] = d->y_stride[k]; }
    P.x_off = d->x_off; P.y_off = d->y_off;
    P.lam_mode = d->lam_mode;
    const long long need = kron_work_len(P);
    IGX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    double *own = nullptr;
    if (need > 0 && !d_work) {
        IGX_HIP(hipMalloc((void **)&own, 2 * (size_t)need * sizeof(double)));
        d_work = own;
    } else if (need > 0 && work_len < 2 * need) {
        set_error("igx_kron_apply_d: work buffer of %lld doubles, %lld needed", (long long)work_len, 2 * need);
        return IGX_ERR_ARG;
    }
    double *W[2] = {d_work, d_work ? d_work + need : nullptr};
    int rc = launch_kron_plan(st, P, d_x, d_y, W);
    hipError_t e = hipStreamSynchronize(st);
    (void)hipFree(own);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("igx_kron_apply_d: %s", hipGetErrorString(e)); return IGX_ERR_HIP; }
    return IGX_OK;
}

} // extern "C"
