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
//   k_csr_spmm2  the block product of the multipatch eigen-solver over the same CSR pattern: K and M times a block of interleaved
//              columns in one pass (k_spmm2 is its structured twin of section 22).
//   k_block_spmv  the product of a vector-valued form's NC x NC blocks (NC = 2, 3), which share the patch's layout: one group per
//              scalar row computes the NC outputs (igx_solver_create_block).
//   vector     fused CG updates and fixed-order two-pass dot products (fixed grid, fixed trees): two solves of the same
//              system give bit-identical results.  alpha and beta stay in device memory.
//   BiCGStab   for non-symmetric matrices (igx_solver_create_general / igx_solver_set_method): the same SpMVs and
//              preconditioners, fused p / s / x-r updates that emit their dot partials, and k_fin_bicg for rho, alpha, omega,
//              the stop and breakdown on the device.
// Host side: one dispatch table per SpMV family (with_spmv_kernel, with_csr_spmv_kernel) names the instantiations, for the launch
// and the occupancy query alike; one fast-diagonalization block (FastDiag) is the Kronecker preconditioner of a patch and the
// local solve of every Schwarz patch; igx_solver_solve forms the lifted right-hand side and hands over to solve_cg or
// solve_bicgstab.
#include "igx_internal.h"
#include "mg_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace igx;

namespace {

constexpr int BLOCK = 256;
constexpr int NB_VEC = 1024;             // blocks of the vector kernels (and most partial sums of a dot product)
constexpr int NB_SPMV_MAX = 8192;        // blocks of the SpMV (grid-stride over rows): what is resident at once, at most this
enum { SC_PQ = 0, SC_RZ, SC_RR, SC_ALPHA, SC_BETA, SC_N = 8 };
enum { FIN_ALPHA = 0, FIN_BETA = 1, FIN_INIT = 2 };

// per-axis tables of the value layout; a 2D patch is a 3D one with a one-dof outer axis
struct Geom {
    int N[3];
    const int *jlo[3], *jhi[3], *rp[3];
    long long S1, S2;
    long long nrows;
};

__device__ __forceinline__ double block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    const double s = sh[0];
    __syncthreads();
    return s;
}

// what a row needs from the per-axis tables: loaded one row ahead, while the values of the current row are in flight
struct RowHdr {
    int fr, l0, l1, l2, c0, c1, c2, r0, r1, r2;
};

__device__ __forceinline__ RowHdr row_hdr(const Geom &g, const uint8_t *freem, long long I)
{
    RowHdr h;
    const int i2 = (int)(I % g.N[2]);
    const long long t = I / g.N[2];
    const int i1 = (int)(t % g.N[1]), i0 = (int)(t / g.N[1]);
    h.fr = freem[I];
    h.l0 = g.jlo[0][i0]; h.l1 = g.jlo[1][i1]; h.l2 = g.jlo[2][i2];
    h.c0 = g.jhi[0][i0]; h.c1 = g.jhi[1][i1]; h.c2 = g.jhi[2][i2];
    h.r0 = g.rp[0][i0]; h.r1 = g.rp[1][i1]; h.r2 = g.rp[2][i2];
    return h;
}

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

// the NC x NC blocks of a vector-valued form: v[p * NC + q] holds block (p, q) (test component p, trial component q) in the
// patch's structured layout, or is null (a block that was never assembled: zero)
struct BlockVals {
    const double *v[9];
};

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

// the box of one patch in its local dofs (3D; a 2D patch has a one-dof outer axis) and its local-to-global map
struct BoxMap {
    int lo[3], nb[3], N[3];
    long long nbox;
    const int32_t *l2g;
};

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
// DIRK time stepping (igx_solver_create_parabolic)
typedef double dbl2 __attribute__((ext_vector_type(2)));
constexpr int AXPBY_U = 4;                       // pairs of M and K values of each lane in flight
constexpr int COMB_MAX = 8;                      // vectors of one k_dirk_rhs pass

// C = alpha M + beta K over the 64-bit value range (24 bytes per value): 16-byte loads, non-temporal (M and K are not read again
// by this pass), 16-byte stores; the odd last value by one lane
__global__ void __launch_bounds__(BLOCK) k_vals_axpby(long long n, double alpha, const double *__restrict__ M, double beta,
                                                      const double *__restrict__ K, double *__restrict__ C)
{
    const long long n2 = n / 2, stride = (long long)gridDim.x * BLOCK;
    const dbl2 *M2 = reinterpret_cast<const dbl2 *>(M), *K2 = reinterpret_cast<const dbl2 *>(K);
    dbl2 *C2 = reinterpret_cast<dbl2 *>(C);
    const dbl2 zero = {0.0, 0.0};
    for (long long i0 = (long long)blockIdx.x * BLOCK + threadIdx.x; i0 < n2; i0 += AXPBY_U * stride) {
        dbl2 m[AXPBY_U], k[AXPBY_U];
#pragma unroll
        for (int u = 0; u < AXPBY_U; ++u) {
            const bool in = i0 + u * stride < n2;
            m[u] = in ? __builtin_nontemporal_load(M2 + i0 + u * stride) : zero;
            k[u] = in ? __builtin_nontemporal_load(K2 + i0 + u * stride) : zero;
        }
#pragma unroll
        for (int u = 0; u < AXPBY_U; ++u)
            if (i0 + u * stride < n2) C2[i0 + u * stride] = alpha * m[u] + beta * k[u];
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) C[n - 1] = alpha * M[n - 1] + beta * K[n - 1];
}

// a linear combination of at most COMB_MAX vectors, coefficients by value
struct Comb {
    int nv;
    double c[COMB_MAX];
    const double *v[COMB_MAX];
};

// out = sum_k c[k] v[k], k = 0 .. nv-1 in this order (the stage right-hand side  M x + tau sum_j a_ij F_j + tau gamma f, and
// y = x + ext(g)): one pass, (nv + 1) 8 bytes per entry
__global__ void k_dirk_rhs(long long n, const Comb L, double *out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < COMB_MAX; ++k)
            if (k < L.nv) a += L.c[k] * L.v[k][i];
        out[i] = a;
    }
}

// The error estimate of an adaptive step fused with its weighted norm:  e_j = sum_k c[k] v[k][j],
// part[block] = sum over the free dofs of (e_j / (tol + tol |x_j|))^2.  Fixed dofs are left out by a select, so whatever finite or
// non-finite value e has there does not reach the sum.  One grid-stride pass of (nv + 1) 8 bytes + the mask byte per dof; the
// partials are finished by k_fin in its fixed order.  V2: every vector, x and the mask are 16-byte aligned, so that two dofs are
// one 16-byte load of each vector and one 2-byte load of the mask; the odd last dof is lane 0's of block 0
template <bool V2>
__global__ void __launch_bounds__(BLOCK) k_err_norm(long long n, const Comb L, const double *__restrict__ x,
                                                    const uint8_t *__restrict__ freem, double tol, double *part)
{
    __shared__ double sh[BLOCK];
    const long long stride = (long long)gridDim.x * BLOCK, t0 = (long long)blockIdx.x * BLOCK + threadIdx.x;
    double s = 0.0;
    auto term = [&](double e, double xj, bool free) {
        const double q = e / (tol + tol * fabs(xj));
        return free ? q * q : 0.0;
    };
    if (V2) {
        const long long n2 = n / 2;
        const dbl2 *x2 = reinterpret_cast<const dbl2 *>(x);
        const unsigned short *m2 = reinterpret_cast<const unsigned short *>(freem);
        for (long long i = t0; i < n2; i += stride) {
            dbl2 e = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < COMB_MAX; ++k)
                if (k < L.nv) e += L.c[k] * reinterpret_cast<const dbl2 *>(L.v[k])[i];
            const dbl2 xv = x2[i];
            const unsigned m = m2[i];
            s += term(e.x, xv.x, (m & 0xffu) != 0);
            s += term(e.y, xv.y, (m >> 8) != 0);
        }
        if ((n & 1) && t0 == 0) {
            double e = 0.0;
#pragma unroll
            for (int k = 0; k < COMB_MAX; ++k)
                if (k < L.nv) e += L.c[k] * L.v[k][n - 1];
            s += term(e, x[n - 1], freem[n - 1] != 0);
        }
    } else {
        for (long long i = t0; i < n; i += stride) {
            double e = 0.0;
#pragma unroll
            for (int k = 0; k < COMB_MAX; ++k)
                if (k < L.nv) e += L.c[k] * L.v[k][i];
            s += term(e, x[i], freem[i] != 0);
        }
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the eigenvalue slots of the packed fast-diagonalization factors from the raw eigenvalues kept beside them:
// lam'_k = scale lam_k + shift  (C = M + tau gamma K: scale = tau gamma, shift = 1/dim; M: scale = 0)
struct LamSlots {
    int nax;
    int m[3];
    long long slot[3], raw[3];               // offsets of lam'_k in the factor buffer and of lam_k in the raw one
};

__global__ void k_kron_lam(const LamSlots L, const double *__restrict__ raw, double *fac, double scale, double shift)
{
    for (int k = 0; k < L.nax; ++k)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.m[k]; i += gridDim.x * blockDim.x)
            fac[L.slot[k] + i] = scale * raw[L.raw[k] + i] + shift;
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

// the contractions of a whole Kronecker product: x (strided) -> work -> ... -> y (strided)
struct KronPlan {
    int dim;
    int m[3], n[3];
    const double *B[3];
    long long batch;
    long long x_off, x_stride[4], y_off, y_stride[4];
    int lam_mode;
    const double *lam[3];
};

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

// ---------------------------------------------------------------------------------------------
// the fast-diagonalization inverse  (x) U_k . D^-1 . (x) U_k^T  of one box (m[k] dofs on axis k): x is read and y written at
// io_off with the strides io_stride, in between compact box vectors.  Its factors, per axis U_k^T | U_k | lam_k, lie in one
// device buffer (pack_fastdiag).
struct FastDiag {
    int dim;
    KronPlan kl, kr;                     // (x) U_k^T with D^-1, then (x) U_k
};

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

} // namespace

// ---------------------------------------------------------------------------------------------
// one patch of the Schwarz preconditioner: its box and its fast-diagonalization inverse (compact box vectors in and out)
struct SwPatch {
    BoxMap map;
    FastDiag F;
};

// the session of the block eigen-solver (igx_solver_eig_*): blocks of n rows and mb interleaved columns
enum { EIG_NBLK = 10, EIG_NSCRATCH = 6, EIG_MB_MAX = 16 };
struct EigState {
    int m = 0, mb = 0;                        // columns of the session's blocks and their row stride (0: no session)
    int timed = 0;
    double *d_blocks = nullptr;               // EIG_NBLK + EIG_NSCRATCH blocks of n * mb
    double *blk[EIG_NBLK + EIG_NSCRATCH] = {};   // (a combination writes scratch blocks, then swaps the pointers)
    double *d_tmp = nullptr;                  // one block of n * EIG_MB_MAX: the masked input of the _d products
    double *d_gpart = nullptr, *d_small = nullptr;   // partial sums; Gram result | coefficients | lam | norms
    double *d_dinv = nullptr;                 // Jacobi: 1 / diag(K) on the free dofs
    double *d_fac = nullptr, *d_W = nullptr;  // Kronecker: packed factors, two work buffers of nbox * EIG_MB_MAX
    int precond = IGX_PRECOND_NONE;
    int box_lo[3] = {}, box_nb[3] = {1, 1, 1}, lam_mode = 0;
    int nb_spmm[3][2] = {};                   // resident blocks of the block product per width and matrix count (0: not asked yet)
    hipEvent_t ev[2] = {};
    bool have_ev = false;
    igx_eig_info info{};
};

// x -= d (the Newton update; d vanishes on the fixed dofs)
__global__ void k_sub(long long n, double *x, const double *d)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] -= d[i];
}

struct igx_solver {
    igx_ctx *ctx = nullptr;
    igx_patch *pt = nullptr;                  // the patch of a patch solver, or
    igx_multipatch *mp = nullptr;             // the global sums of a multipatch solver
    unsigned long long gen = 0;               // mp->generation the solver was made over
    int kind = 0;
    int dim = 0;
    int N[3] = {1, 1, 1};                    // dofs per axis of the patch (dim of them)
    long long n = 0;
    Geom g{};
    int gw = 64;
    int nb_spmv = 1;                          // SpMV blocks resident on the device at once (fixed per solver: fixed summation order)
    int *d_tab = nullptr;
    uint8_t *d_mask = nullptr;
    std::vector<uint8_t> h_free;
    std::vector<long long> fixed;
    double *d_vec = nullptr;                  // x | r | p | q | z | b | w | dinv, n each
    double *x = nullptr, *r = nullptr, *p = nullptr, *q = nullptr, *z = nullptr, *b = nullptr, *w = nullptr, *dinv = nullptr;
    double *d_part = nullptr;                 // 2 x NB_SPMV_MAX partial sums
    double *d_sc = nullptr;                   // SC_N scalars
    int precond = IGX_PRECOND_NONE;
    FastDiag kron{};                          // the Kronecker preconditioner on the free box of the full-length vectors
    double *d_kron = nullptr;                 // U_k^T | U_k | lam_k (Schwarz: of every patch)
    double *d_W = nullptr;                    // two work buffers
    long long wlen = 0;
    std::vector<SwPatch> sw;                  // Schwarz: the patches with a non-empty box
    double *d_box = nullptr;                  // Schwarz: one patch's box (gathered residual, then the local correction)
    hipEvent_t ev[6] = {};
    bool have_ev = false;
    // BiCGStab (allocated only once a solver is switched to it): v = q, p^ = z; r^ | s | s^ | t in d_bvec, its scalars in d_bsc
    int method = IGX_METHOD_CG;
    double *d_bvec = nullptr;
    double *rh = nullptr, *sv = nullptr, *sh = nullptr, *t = nullptr;
    double *d_bsc = nullptr;
    int breakdown = 0;                        // reason of the last BiCGStab solve (IGX_BREAKDOWN_*), 0 if none
    hipEvent_t bev[8] = {};
    bool have_bev = false;
    // block solver of a vector-valued form (igx_solver_create_block): ncomp components of g.nrows dofs each, n = ncomp g.nrows
    int ncomp = 1;
    bool symmetric = false;                   // made as symmetric: CG allowed
    double *blk[9] = {};                      // block (p, q) at p * ncomp + q, taken from the patch (owned), or null
    FastDiag bkron[3] = {};                   // per component: the fast-diagonalization inverse on its free box (in d_bkron[c])
    double *d_bkron[3] = {};
    // parabolic solver (igx_solver_create_parabolic): M and K taken from the patch (IGX_ROLE_*), C = M + tau gamma K formed by
    // igx_solver_set_dirk; the SpMV, Jacobi and the solves act on C
    bool parabolic = false;
    double *pv[3] = {};                       // M | K | C, owned
    long long nvals[2] = {};                  // values of M and K
    bool c_formed = false;
    int stages = 0;
    double dirk_A[(IGX_DIRK_MAX_STAGES + 1) * IGX_DIRK_MAX_STAGES] = {};
    double tau = 0.0, gamma = 0.0;
    float axpby_ms = 0.0f;                    // device time of the last k_vals_axpby
    double *d_dirk = nullptr;                 // xs | Mx | f | y | F_0 .. F_{stages-1}, n each (allocated by the first run)
    hipEvent_t dev[6] = {};
    bool have_dev = false;
    // adaptive stepping session (igx_solver_set_stepper .. igx_solver_step_accept)
    double c_tg = 0.0;                        // the tau gamma of the C on the device (c_formed)
    const double *vals_sel = nullptr;         // the values the SpMV and Jacobi read instead of C (the mass solve: M)
    int family = -1;                          // IGX_STEPPER_*, -1: no stepper set
    int st_stages = 0;
    bool st_bhat = false;
    double st_A[(IGX_DIRK_MAX_STAGES + 1) * IGX_DIRK_MAX_STAGES] = {};    // DIRK: b the last row; Rosenbrock: stages rows
    double st_G[IGX_DIRK_MAX_STAGES * IGX_DIRK_MAX_STAGES] = {};
    double st_b[IGX_DIRK_MAX_STAGES] = {}, st_bh[IGX_DIRK_MAX_STAGES] = {};
    double st_gamma = 0.0;
    int step_precond = -1;                    // the session's preconditioner (IGX_PRECOND_*), -1: not set (or replaced since)
    LamSlots lam_slots{};
    double *d_lamraw = nullptr;               // the raw eigenvalues lam_k, axis after axis
    int pc_vals = -1;                         // what the preconditioner data was last made for: 0 M, 2 C (-1: nothing), with
    double pc_tg = 0.0;                       // this tau gamma
    double *d_wg = nullptr;                   // ext(g) of the session (allocated by the first igx_solver_step_begin)
    bool step_live = false, have_mx = false, have_F0 = false, have_cand = false;
    double *sx = nullptr, *smx = nullptr, *sfv = nullptr, *sy = nullptr, *sF[IGX_DIRK_MAX_STAGES] = {};
    // multigrid (igx_solver_set_mg_*, multigrid.hip): this solver's level of the hierarchy, or null
    igx::MgLevel *mg = nullptr;
    // block eigen-solver (igx_solver_eig_*): made by its first call, or null
    EigState *eig = nullptr;
    double *d_mass = nullptr;                 // a multipatch solver's second matrix (igx_solver_set_mass_d), owned
};

namespace {

int check_values(const igx_solver *s, const char *what)
{
    if (s->ncomp > 1) {                       // (the blocks are the solver's own: only a missing diagonal one is refused)
        for (int c = 0; c < s->ncomp; ++c)
            if (!s->blk[c * s->ncomp + c]) {
                set_error("%s: diagonal block (%d, %d) missing: take it first (igx_solver_take_block)", what, c, c);
                return IGX_ERR_ARG;
            }
        return IGX_OK;
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
        if (!s->c_formed) {
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
    return s->vals_sel ? s->vals_sel : s->pv[2];       // (vals_sel: M, during the mass solve of an embedded DIRK attempt)
}

unsigned spmv_blocks(const igx_solver *s)
{
    const long long groups = BLOCK / s->gw, rows = s->n / s->ncomp;      // (a block solver: one group per scalar row)
    return (unsigned)std::max<long long>(1, std::min<long long>(s->nb_spmv, (rows + groups - 1) / groups));
}

// y = free ? (b ? b : 0) + sign A x : 0 (and the partials of pd.y): k_spmv on a patch's values, k_csr_spmv on a multipatch's sums,
// k_block_spmv on the blocks of a block solver
int spmv(hipStream_t st, const igx_solver *s, const double *x, const double *b, double sign, double *y, const double *pd, double *part)
{
    const unsigned nb = spmv_blocks(s);
    if (s->mp) {
        const igx_multipatch *m = s->mp;
        with_csr_spmv_kernel(s->gw, [&](auto k) {
            k<<<nb, BLOCK, 0, st>>>(s->n, m->d_indptr, m->d_indices, m->d_vals, s->d_mask, x, b, sign, y, pd, part);
        });
    } else if (s->ncomp > 1) {
        BlockVals A{};
        for (int k = 0; k < s->ncomp * s->ncomp; ++k) A.v[k] = s->blk[k];
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
int apply_kron(hipStream_t st, igx_solver *s, const double *r, double *z)
{
    double *W[2] = {s->d_W, s->d_W + s->wlen};
    if (s->ncomp > 1) {
        for (int c = 0; c < s->ncomp; ++c)
            if (int rc = apply_fastdiag(st, s->bkron[c], r, z, W)) return rc;
        return IGX_OK;
    }
    return apply_fastdiag(st, s->kron, r, z, W);
}

// z = sum_p X_p M_p B_p M_p X_p^T r: per patch, in patch order, gather the box, the two Kronecker products, add back on the free dofs
int apply_schwarz(hipStream_t st, igx_solver *s, const double *r, double *z)
{
    IGX_HIP(hipMemsetAsync(z, 0, (size_t)s->n * sizeof(double), st));
    double *W[2] = {s->d_W, s->d_W + s->wlen};
    for (const SwPatch &P : s->sw) {
        const unsigned nb = (unsigned)((P.map.nbox + 255) / 256);
        k_box_gather<<<nb, 256, 0, st>>>(P.map, s->d_mask, r, s->d_box);
        IGX_HIP(hipGetLastError());
        if (int rc = apply_fastdiag(st, P.F, s->d_box, s->d_box, W)) return rc;
        k_box_scatter<<<nb, 256, 0, st>>>(P.map, s->d_mask, s->d_box, z);
        IGX_HIP(hipGetLastError());
    }
    return IGX_OK;
}

// the preconditioners applied by kernels of their own (Kronecker, Schwarz); Jacobi is fused into k_update
int apply_dense(hipStream_t st, igx_solver *s, const double *r, double *z)
{
    if (s->precond == IGX_PRECOND_MG) return mg_apply(st, s, r, z);
    return s->precond == IGX_PRECOND_SCHWARZ ? apply_schwarz(st, s, r, z) : apply_kron(st, s, r, z);
}

int spmv_occupancy(const igx_solver *s)
{
    int per_cu = 0;
    auto occupancy = [&](auto k) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, BLOCK, 0); };
    const hipError_t eo = s->mp ? with_csr_spmv_kernel(s->gw, occupancy)
                                : s->ncomp > 1 ? with_block_spmv_kernel(s->gw, s->ncomp, occupancy) : with_spmv_kernel(s->gw, occupancy);
    if (eo != hipSuccess) { (void)hipGetLastError(); per_cu = 1; }
    return (int)std::min<long long>(NB_SPMV_MAX, (long long)std::max(1, per_cu) * std::max(1, s->ctx->ncu));
}

void free_solver(igx_solver *s)
{
    mg_free(s);
    if (EigState *e = s->eig) {
        (void)hipFree(e->d_blocks); (void)hipFree(e->d_tmp); (void)hipFree(e->d_gpart); (void)hipFree(e->d_small);
        (void)hipFree(e->d_dinv); (void)hipFree(e->d_fac); (void)hipFree(e->d_W);
        if (e->have_ev)
            for (auto &ev : e->ev) (void)hipEventDestroy(ev);
        delete e;
    }
    (void)hipFree(s->d_tab); (void)hipFree(s->d_mask); (void)hipFree(s->d_vec); (void)hipFree(s->d_part); (void)hipFree(s->d_sc);
    (void)hipFree(s->d_kron); (void)hipFree(s->d_W); (void)hipFree(s->d_box);
    (void)hipFree(s->d_bvec); (void)hipFree(s->d_bsc); (void)hipFree(s->d_mass);
    for (double *v : s->blk) (void)hipFree(v);
    for (double *v : s->d_bkron) (void)hipFree(v);
    for (double *v : s->pv) (void)hipFree(v);
    (void)hipFree(s->d_dirk); (void)hipFree(s->d_lamraw); (void)hipFree(s->d_wg);
    if (s->have_dev)
        for (auto &e : s->dev) (void)hipEventDestroy(e);
    if (s->have_ev)
        for (auto &e : s->ev) (void)hipEventDestroy(e);
    if (s->have_bev)
        for (auto &e : s->bev) (void)hipEventDestroy(e);
    delete s;
}

// the dof mask from the fixed list (s->n set); false with igx_last_error on a bad list
bool set_fixed(igx_solver *s, const int64_t *fixed, int64_t nfixed, const char *what)
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
int init_vectors(igx_solver *s, const char *what)
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
    if (s->d_bvec) return IGX_OK;
    const size_t n = (size_t)s->n;
    if (hipMalloc((void **)&s->d_bvec, 4 * n * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&s->d_bsc, BS_N * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(s->d_bvec); s->d_bvec = nullptr;
        set_error("%s: out of device memory (%.3f GB)", what, 4.0 * 8 * n / 1e9);
        return IGX_ERR_NOMEM;
    }
    hipError_t e = hipMemsetAsync(s->d_bvec, 0, 4 * n * sizeof(double), s->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return IGX_ERR_HIP; }
    s->rh = s->d_bvec; s->sv = s->d_bvec + n; s->sh = s->d_bvec + 2 * n; s->t = s->d_bvec + 3 * n;
    for (auto &ev : s->bev)
        if (hipEventCreate(&ev) != hipSuccess) { set_error("%s: hipEventCreate failed", what); return IGX_ERR_HIP; }
    s->have_bev = true;
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
int solve_cg(hipStream_t st, igx_solver *s, double bnorm, double tol, int maxiter, int check_every, int timed, igx_solve_info &inf)
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
int solve_bicgstab(hipStream_t st, igx_solver *s, double bnorm, double tol, int maxiter, int check_every, int timed, igx_solve_info &inf)
{
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    const unsigned nbv = vec_blocks(n), nbs = spmv_blocks(s);
    double *pA = s->d_part, *pB = s->d_part + NB_SPMV_MAX;
    double *pC = pA + NB_VEC;                    // (vector kernels write at most NB_VEC partials into pA: pC follows them)
    const bool dense = s->precond == IGX_PRECOND_KRON || s->precond == IGX_PRECOND_SCHWARZ, jac = s->precond == IGX_PRECOND_JACOBI;
    double *v = s->q;
    double *ph = (dense || jac) ? s->z : s->p, *sh = (dense || jac) ? s->sh : s->sv;
    const double *dinv = jac ? s->dinv : nullptr;
    const double stop = tol * bnorm;
    IGX_HIP(hipMemsetAsync(s->d_bsc, 0, BS_N * sizeof(double), st));
    IGX_HIP(hipMemsetAsync(s->sh, 0, nbytes, st));
    IGX_HIP(hipMemsetAsync(s->t, 0, nbytes, st));
    IGX_HIP(hipMemcpyAsync(s->rh, s->r, nbytes, hipMemcpyDeviceToDevice, st));       // r^ = r0
    k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->r, s->r, nullptr, nullptr, pA, nullptr);
    k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbv, nullptr, 0, nullptr, s->d_bsc, FB_INIT, stop);
    IGX_HIP(hipGetLastError());
    double h[BS_N] = {};
    auto readback = [&]() -> int {
        IGX_HIP(hipMemcpyAsync(h, s->d_bsc, sizeof(h), hipMemcpyDeviceToHost, st));
        IGX_HIP(hipStreamSynchronize(st));
        return IGX_OK;
    };
    if (int rc = readback()) return rc;
    hipEvent_t *E = s->bev;
    for (int it = 0; h[BS_DONE] == 0.0 && it < maxiter;) {
        ++it;
        if (timed) IGX_HIP(hipEventRecord(E[0], st));
        k_bicg_p<<<nbv, BLOCK, 0, st>>>(n, s->r, s->p, v, dinv, ph, s->rh, s->d_bsc);
        IGX_HIP(hipGetLastError());
        if (timed) IGX_HIP(hipEventRecord(E[1], st));
        if (dense) { if (int rc = apply_dense(st, s, s->p, ph)) return rc; }
        if (timed) IGX_HIP(hipEventRecord(E[2], st));
        if (int rc = spmv(st, s, ph, nullptr, 1.0, v, s->rh, pA)) return rc;
        if (timed) IGX_HIP(hipEventRecord(E[3], st));
        k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbs, nullptr, 0, nullptr, s->d_bsc, FB_ALPHA, stop);
        k_bicg_s<<<nbv, BLOCK, 0, st>>>(n, s->r, v, s->sv, dinv, sh, s->d_bsc, pA, pB);
        k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbv, pB, nbv, nullptr, s->d_bsc, FB_S, stop);
        IGX_HIP(hipGetLastError());
        if (timed) IGX_HIP(hipEventRecord(E[4], st));
        if (dense) { if (int rc = apply_dense(st, s, s->sv, sh)) return rc; }
        if (timed) IGX_HIP(hipEventRecord(E[5], st));
        if (int rc = spmv(st, s, sh, nullptr, 1.0, s->t, s->sv, pA)) return rc;
        if (timed) IGX_HIP(hipEventRecord(E[6], st));
        k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->t, s->t, nullptr, nullptr, pB, nullptr);
        k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbs, pB, nbv, nullptr, s->d_bsc, FB_OMEGA, stop);
        k_bicg_xr<<<nbv, BLOCK, 0, st>>>(n, s->x, s->r, ph, sh, s->sv, s->t, s->rh, s->d_bsc, pA, pB, pC);
        k_fin_bicg<<<1, BLOCK, 0, st>>>(pA, nbv, pB, nbv, pC, s->d_bsc, FB_RHO, stop);
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
    s->breakdown = (int)h[BS_REASON];
    return IGX_OK;
}

bool spd_kind(int kind) { return kind == IGX_MASS || kind == IGX_STIFFNESS; }

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
int init_solver(igx_solver *s, const int64_t *fixed, int64_t nfixed, long long maxlen, const std::vector<int> &tab, const char *what)
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
                        const char *what)
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
    s->ctx = pt->ctx; s->pt = pt; s->kind = kind; s->dim = pt->dim; s->ncomp = ncomp; s->n = ncomp * pt->nrows_total;
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
int check_free_box(const igx_solver *s, long long base, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                   const double *const *lam, int nb[3], const char *what)
{
    const int d = s->dim;
    for (int k = 0; k < d; ++k) {
        if (box_lo[k] < 0 || box_hi[k] > s->N[k] || box_lo[k] >= box_hi[k] || !U[k] || !lam[k]) {
            set_error("%s: bad free box [%d, %d) on axis %d", what, box_lo[k], box_hi[k], k);
            return IGX_ERR_ARG;
        }
        nb[k] = box_hi[k] - box_lo[k];
    }
    long long I = 0;
    int i[3] = {0, 0, 0};
    for (i[0] = 0; i[0] < s->N[0]; ++i[0])
        for (i[1] = 0; i[1] < (d > 1 ? s->N[1] : 1); ++i[1])
            for (i[2] = 0; i[2] < (d > 2 ? s->N[2] : 1); ++i[2], ++I) {
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
                      long long batch = 1)
{
    long long full_stride[4], off = base;
    box_strides(s->dim, s->N, full_stride);
    for (int k = 0; k < s->dim; ++k) off += box_lo[k] * full_stride[k];
    return make_fastdiag(s->dim, nb, d_fac, full_stride, off, lam_mode, batch);
}

// The Kronecker inverse on the free box of the component at `base` of a patch solver, for the entry point `what`: checks the
// arguments, packs the factors and puts them on the device at d_fac in place of the previous ones (synchronised before and
// after).  *reset (or null) becomes IGX_PRECOND_NONE before anything is freed, whatever fails later.  nb out
int box_fastdiag_setup(igx_solver *s, long long base, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                       const double *const *lam, int lam_mode, const char *what, int *reset, double *&d_fac, int nb[3])
{
    if (!box_lo || !box_hi || !U || !lam) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (lam_mode != IGX_KRON_SUM && lam_mode != IGX_KRON_PRODUCT) { set_error("%s: unknown lam_mode %d", what, lam_mode); return IGX_ERR_ARG; }
    nb[0] = nb[1] = nb[2] = 1;
    if (int rc = check_free_box(s, base, box_lo, box_hi, U, lam, nb, what)) return rc;
    std::vector<double> h;
    pack_fastdiag(h, s->dim, nb, U, lam);
    if (reset) *reset = IGX_PRECOND_NONE;
    IGX_HIP(hipStreamSynchronize(s->ctx->stream));
    if (int rc = upload_replacing(s->ctx->stream, h, d_fac)) return rc;
    IGX_HIP(hipStreamSynchronize(s->ctx->stream));       // (h goes away)
    return IGX_OK;
}

} // namespace

// what multigrid.hip sees of a solver (mg_internal.h)
namespace igx {

SolverRef solver_ref(const igx_solver *s)
{
    return SolverRef{s->ctx, s->mp, s->n, s->gw, s->d_mask, s->h_free.data(), s->precond, s->method};
}

MgLevel *&solver_mg(igx_solver *s) { return s->mg; }

void solver_drop_mg_precond(igx_solver *s)
{
    if (s->precond == IGX_PRECOND_MG) s->precond = IGX_PRECOND_NONE;
}

int solver_check_sums(const igx_solver *s, const char *what)
{
    if (!s->mp) { set_error("%s: a multigrid level needs a multipatch solver", what); return IGX_ERR_UNSUPPORTED; }
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

int igx_solver_last_breakdown(const igx_solver *s) { return s ? s->breakdown : 0; }

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
    if (s->ncomp < 2) { set_error("%s: not a block solver (igx_solver_create_block)", what); return IGX_ERR_ARG; }
    if (p < 0 || p >= s->ncomp || q < 0 || q >= s->ncomp) { set_error("%s: block (%d, %d) of %d components", what, p, q, s->ncomp); return IGX_ERR_ARG; }
    double *&dst = s->blk[p * s->ncomp + q];
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

int igx_solver_set_block_kron(igx_solver *s, int comp, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                              const double *const *lam, int mode)
{
    const char *what = "igx_solver_set_block_kron";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (s->ncomp < 2) { set_error("%s: not a block solver (igx_solver_create_block)", what); return IGX_ERR_ARG; }
    if (comp < 0 || comp >= s->ncomp) { set_error("%s: component %d of %d", what, comp, s->ncomp); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    const long long base = (long long)comp * s->g.nrows;
    int nb[3];
    // (a Kronecker preconditioner in use is dropped: selected again by igx_solver_set_precond)
    if (int rc = box_fastdiag_setup(s, base, box_lo, box_hi, U, lam, mode, what, s->precond == IGX_PRECOND_KRON ? &s->precond : nullptr,
                                    s->d_bkron[comp], nb)) return rc;
    const long long nbox = (long long)nb[0] * nb[1] * nb[2];
    if (nbox > s->wlen)                            // the two work buffers fit the largest box of any component
        if (int rc = alloc_fastdiag_work(s, nbox)) return rc;
    s->bkron[comp] = box_fastdiag(s, base, box_lo, nb, s->d_bkron[comp], mode);
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
    s->step_precond = -1;                                // (a stepping session's preconditioner data is replaced: set it again)
    s->pc_vals = -1;
    if (precond == IGX_PRECOND_NONE) { s->precond = precond; return IGX_OK; }
    if (precond == IGX_PRECOND_JACOBI) {
        if (int rc = check_values(s, "igx_solver_set_precond")) return rc;
        if (s->mp) k_csr_diag<<<(unsigned)((s->n + 255) / 256), 256, 0, st>>>(s->n, s->mp->d_indptr, s->mp->d_indices, s->mp->d_vals, s->d_mask, s->dinv);
        else if (s->ncomp > 1) {
            const long long N = s->g.nrows;                   // component c: the diagonal of block (c, c) at offset c N
            for (int c = 0; c < s->ncomp; ++c)
                k_diag<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(s->g, s->blk[c * s->ncomp + c], s->d_mask + c * N, s->dinv + c * N);
        } else k_diag<<<(unsigned)((s->n + 255) / 256), 256, 0, st>>>(s->g, patch_values(s), s->d_mask, s->dinv);
        IGX_HIP(hipGetLastError());
        IGX_HIP(hipStreamSynchronize(st));
        s->precond = precond;
        return IGX_OK;
    }
    if (precond == IGX_PRECOND_SCHWARZ) {
        if (!s->mp) { set_error("igx_solver_set_precond: the Schwarz preconditioner needs a multipatch solver"); return IGX_ERR_UNSUPPORTED; }
        if (s->sw.empty() || !s->d_W) { set_error("igx_solver_set_precond: set the Schwarz factors up first (igx_solver_set_schwarz)"); return IGX_ERR_ARG; }
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
            if (!s->d_bkron[c]) {
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

int igx_solver_set_schwarz(igx_solver *s, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                           const double *const *lam, int lam_mode)
{
    if (!s) { set_error("igx_solver_set_schwarz: null solver"); return IGX_ERR_ARG; }
    if (!s->mp) { set_error("igx_solver_set_schwarz: the Schwarz preconditioner needs a multipatch solver"); return IGX_ERR_UNSUPPORTED; }
    const igx_multipatch *mp = s->mp;
    if (!mp->injective) {
        set_error("igx_solver_set_schwarz: a local-to-global map is not injective (two dofs of one patch share a global dof); "
                  "use IGX_PRECOND_JACOBI");
        return IGX_ERR_UNSUPPORTED;
    }
    if (!box_lo || !box_hi || !U || !lam) { set_error("igx_solver_set_schwarz: null argument"); return IGX_ERR_ARG; }
    if (lam_mode != IGX_KRON_SUM && lam_mode != IGX_KRON_PRODUCT) { set_error("igx_solver_set_schwarz: unknown lam_mode %d", lam_mode); return IGX_ERR_ARG; }
    // per patch with a non-empty box its map and, per axis, U_k^T | U_k | lam_k at fac[j] in h
    std::vector<SwPatch> sw;
    std::vector<size_t> fac;
    std::vector<double> h;
    long long wlen = 1;
    for (int p = 0; p < mp->np; ++p) {
        const auto &P = mp->pp[p];
        bool empty = false;
        for (int k = 0; k < P.dim; ++k) {
            const int lo = box_lo[p * 3 + k], hi = box_hi[p * 3 + k];
            if (lo < 0 || hi > P.N[k] || lo > hi) {
                set_error("igx_solver_set_schwarz: patch %d: bad box [%d, %d) on axis %d of %d dofs", p, lo, hi, k, P.N[k]);
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
            if (!U[p * 3 + k] || !lam[p * 3 + k]) { set_error("igx_solver_set_schwarz: patch %d: factor of axis %d missing", p, k); return IGX_ERR_ARG; }
            W.map.lo[off + k] = box_lo[p * 3 + k]; W.map.nb[off + k] = m; W.map.N[off + k] = P.N[k];
            W.map.nbox *= m;
        }
        W.map.l2g = P.d_l2g;
        W.F.dim = P.dim;
        fac.push_back(pack_fastdiag(h, P.dim, W.map.nb + off, U + p * 3, lam + p * 3));
        wlen = std::max(wlen, W.map.nbox);
        sw.push_back(W);
    }
    if (sw.empty()) { set_error("igx_solver_set_schwarz: every patch box is empty"); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipStreamSynchronize(st));
    (void)hipFree(s->d_box); s->d_box = nullptr;
    s->sw.clear();
    if (s->precond == IGX_PRECOND_SCHWARZ) s->precond = IGX_PRECOND_NONE;
    if (int rc = upload_replacing(st, h, s->d_kron)) return rc;
    if (int rc = alloc_fastdiag_work(s, wlen)) return rc;
    IGX_HIP(hipMalloc((void **)&s->d_box, (size_t)wlen * sizeof(double)));
    for (size_t j = 0; j < sw.size(); ++j) {
        const int d = sw[j].F.dim;
        const int *m = sw[j].map.nb + (3 - d);
        long long stride[4];                            // compact box vectors in and out
        box_strides(d, m, stride);
        sw[j].F = make_fastdiag(d, m, s->d_kron + fac[j], stride, 0, lam_mode);
    }
    IGX_HIP(hipStreamSynchronize(st));
    s->sw = std::move(sw);
    s->precond = IGX_PRECOND_SCHWARZ;
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
        k_mask_copy<<<nb, 256, 0, st>>>(s->n, s->d_mask, d_r, s->w);
        if (int rc = mg_apply(st, s, s->w, d_z)) return rc;
        break;
    default: k_mask_copy<<<nb, 256, 0, st>>>(s->n, s->d_mask, d_r, d_z); break;
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
    k_mask_copy<<<(unsigned)((s->n + 255) / 256), 256, 0, st>>>(s->n, s->d_mask, d_x, s->w);
    IGX_HIP(hipGetLastError());
    if (int rc = spmv(st, s, s->w, nullptr, 1.0, d_y, nullptr, nullptr)) return rc;
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

} // extern "C"

namespace {

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
int finish_solve(hipStream_t st, igx_solver *s, const double *gvals, double *u, igx_solve_info *info, igx_solve_info &inf)
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
// multiplies by (a parabolic solver: C, or the values of s->vals_sel) and the preconditioner the one s holds now.
// `from_guess` (with x0_in_x): the stop is relative to the residual the initial guess leaves, ||r|| <= tol ||r0||, as the
// reference's Newton measures it (pyiga/solvers.py:350-354: rtol times the residual at the start value): the solve is then one
// for the increment x - x0, and its tolerance refers to the change of a stage and not to the 1/(tau |F|) times larger state.  A
// guess that meets tol ||R (b - A w)|| already is the solution (no iteration), and the stop is never below
// 100 eps ||R (b - A w)||, which the true residual cannot be seen to pass.
int solve_lifted(hipStream_t st, igx_solver *s, const double *lift, bool x0_in_x, double tol, int maxiter, int check_every, int timed,
                 igx_solve_info &inf, bool from_guess = false)
{
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
    } else k_mask_copy<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, s->d_mask, s->b, s->r);
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
            k_fin<<<1, BLOCK, 0, st>>>(pA, nullptr, nbv, s->d_sc, FIN_INIT);
            IGX_HIP(hipGetLastError());
            IGX_HIP(hipMemcpyAsync(&h_rr, s->d_sc + SC_RR, sizeof(double), hipMemcpyDeviceToHost, st));
            IGX_HIP(hipStreamSynchronize(st));
            IGX_HIP(hipMemsetAsync(s->d_sc, 0, SC_N * sizeof(double), st));
            // (not below what double precision resolves of the true residual: 100 eps ||R (b - A w)||)
            if (std::sqrt(h_rr) > tol * bnorm) bnorm = std::max(std::sqrt(h_rr), 100.0 * 2.220446049250313e-16 * bnorm / tol);
        }
    }
    return s->method == IGX_METHOD_BICGSTAB ? solve_bicgstab(st, s, bnorm, tol, maxiter, check_every, timed, inf)
                                            : solve_cg(st, s, bnorm, tol, maxiter, check_every, timed, inf);
}

} // namespace

extern "C" {

int igx_solver_solve(igx_solver *s, const double *b, const double *gvals, const double *x0, double tol, int maxiter, int check_every,
                     int timed, double *u, igx_solve_info *info)
{
    if (!s || (!b && !s->mp) || (!gvals && !s->fixed.empty()) || !u) { set_error("igx_solver_solve: null argument"); return IGX_ERR_ARG; }
    if (!(tol >= 0.0) || maxiter < 0) { set_error("igx_solver_solve: tol must be >= 0 and maxiter >= 0"); return IGX_ERR_ARG; }
    if (int rc = check_values(s, "igx_solver_solve")) return rc;
    if (check_every < 1) check_every = 1;
    s->breakdown = 0;
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

// --- Newton's method on a patch solver: the iterate, the residual and the Jacobian stay on the device ----
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
    k_diag<<<(unsigned)((s->n + 255) / 256), 256, 0, st>>>(s->g, patch_values(s), s->d_mask, s->dinv);
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
    k_mask_copy<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, s->d_mask, d_v, s->r);
    k_dot2<<<nbv, BLOCK, 0, st>>>(n, s->r, s->r, nullptr, nullptr, s->d_part, nullptr);
    k_fin<<<1, BLOCK, 0, st>>>(s->d_part, nullptr, nbv, s->d_sc, FIN_INIT);
    IGX_HIP(hipGetLastError());
    double h_rr = 0.0;
    IGX_HIP(hipMemcpyAsync(&h_rr, s->d_sc + SC_RR, sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
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
    s->breakdown = 0;
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

// ---------------------------------------------------------------------------------------------
// Parabolic problems: DIRK time stepping of  M u' = f - K u  on the free dofs, u = g on the fixed ones (DESIGN.md section 16;
// pyiga/solvers.py:366-473).  Every implicit stage solves  R C R^T y = R (b_i - C ext(g)),  C = M + tau gamma K,  with
// b_i = M x + tau sum_{j<i} a_ij F_j + tau gamma f  and  F_j = f - K y_j.

namespace {

// a DIRK tableau in the reference's layout ((stages + 1) x stages, b the last row) that every implicit stage of every step solves
// with one matrix: lower triangular, every nonzero diagonal entry one gamma > 0, only row 0 may have a zero diagonal, stiffly
// accurate (b is the last stage row, exactly).  gamma out; false with igx_last_error
bool dirk_ok(int st, const double *A, double tau, double &gamma, const char *what)
{
    if (st < 1 || st > IGX_DIRK_MAX_STAGES) { set_error("%s: %d stages (1 to %d)", what, st, IGX_DIRK_MAX_STAGES); return false; }
    if (!(tau > 0.0) || !std::isfinite(tau)) { set_error("%s: tau must be positive and finite", what); return false; }
    gamma = 0.0;
    for (int i = 0; i <= st; ++i)
        for (int j = 0; j < st; ++j) {
            const double a = A[i * st + j];
            if (!std::isfinite(a)) { set_error("%s: A[%d][%d] is not finite", what, i, j); return false; }
            if (i < st && j > i && a != 0.0) { set_error("%s: A is not lower triangular (A[%d][%d] = %g)", what, i, j, a); return false; }
        }
    for (int i = 0; i < st; ++i) {
        const double a = A[i * st + i];
        if (a == 0.0) {
            if (i > 0) { set_error("%s: zero diagonal in stage %d (only the first stage may be explicit)", what, i); return false; }
            continue;
        }
        if (!(a > 0.0)) { set_error("%s: diagonal A[%d][%d] = %g is not positive", what, i, i, a); return false; }
        if (gamma != 0.0 && a != gamma) { set_error("%s: two diagonal values (%.17g and %.17g): C would change per stage", what, gamma, a); return false; }
        gamma = a;
    }
    if (gamma == 0.0) { set_error("%s: no implicit stage", what); return false; }
    for (int j = 0; j < st; ++j)
        if (A[st * st + j] != A[(st - 1) * st + j]) {
            set_error("%s: the scheme is not stiffly accurate (b differs from the last stage row at %d)", what, j);
            return false;
        }
    return true;
}

// xs | Mx | f | y | F_0 .. F_5 of a parabolic solver, n each (once)
int alloc_dirk_vectors(igx_solver *s, const char *what)
{
    if (s->d_dirk) return IGX_OK;
    const size_t nbytes = (size_t)s->n * sizeof(double);
    if (hipMalloc((void **)&s->d_dirk, (4 + IGX_DIRK_MAX_STAGES) * nbytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: out of device memory (%.3f GB)", what, (4.0 + IGX_DIRK_MAX_STAGES) * nbytes / 1e9);
        return IGX_ERR_NOMEM;
    }
    return IGX_OK;
}

// the buffer of C and the events of the time stepping (once)
int alloc_stage_matrix(igx_solver *s, const char *what)
{
    const long long nv = s->nvals[0];
    if (!s->pv[2]) {
        if (hipMalloc((void **)&s->pv[2], (size_t)nv * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: out of device memory (%.3f GB for C)", what, 8.0 * nv / 1e9);
            return IGX_ERR_NOMEM;
        }
    }
    if (!s->have_dev) {
        for (auto &e : s->dev)
            if (hipEventCreate(&e) != hipSuccess) { set_error("%s: hipEventCreate failed", what); return IGX_ERR_HIP; }
        s->have_dev = true;
    }
    return IGX_OK;
}

// C = M + tg K into the solver's buffer (k_vals_axpby between the events dev[0] and dev[1]; not synchronised)
int form_stage_matrix(hipStream_t st, igx_solver *s, double tg)
{
    const long long nv = s->nvals[0];
    const long long blocks = std::min<long long>((nv / 2 + BLOCK - 1) / BLOCK, 16LL * std::max(1, s->ctx->ncu));
    IGX_HIP(hipEventRecord(s->dev[0], st));
    k_vals_axpby<<<(unsigned)std::max<long long>(1, blocks), BLOCK, 0, st>>>(nv, 1.0, s->pv[0], tg, s->pv[1], s->pv[2]);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipEventRecord(s->dev[1], st));
    return IGX_OK;
}

// timed: the device time since the last lap goes to a bucket; the events ev[mark] and ev[other] alternate
struct PhaseTimer {
    hipEvent_t *ev;
    int mark, other, timed;                  // (the caller records ev[mark] where the first phase starts)
    int lap(hipStream_t st, float &bucket)
    {
        if (!timed) return IGX_OK;
        IGX_HIP(hipEventRecord(ev[other], st));
        IGX_HIP(hipEventSynchronize(ev[other]));
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, ev[mark], ev[other]);
        bucket += ms;
        std::swap(mark, other);
        return IGX_OK;
    }
};

// x0 with g on the fixed dofs to d_x, ext(g) to d_w and f to d_f: the only uploads of a run or a session.  `begin` (or null) is
// recorded ahead of them; synchronised
int upload_start_state(hipStream_t st, const igx_solver *s, const double *f, const double *gvals, const double *x0, double *d_x,
                       double *d_w, double *d_f, hipEvent_t begin)
{
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    std::vector<double> h((size_t)n), w((size_t)n, 0.0);
    for (long long i = 0; i < n; ++i) h[i] = s->h_free[i] ? x0[i] : 0.0;
    for (size_t k = 0; k < s->fixed.size(); ++k) h[s->fixed[k]] = w[s->fixed[k]] = gvals[k];
    if (begin) IGX_HIP(hipEventRecord(begin, st));
    IGX_HIP(hipMemcpyAsync(d_x, h.data(), nbytes, hipMemcpyHostToDevice, st));
    IGX_HIP(hipMemcpyAsync(d_w, w.data(), nbytes, hipMemcpyHostToDevice, st));
    IGX_HIP(hipMemcpyAsync(d_f, f, nbytes, hipMemcpyHostToDevice, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

// the implicit stages of one DIRK step, for igx_solver_dirk_run and the session's igx_solver_step_attempt alike; ok out: every
// stage solve converged (else the chain ends with the stage that did not)
struct StageChain {
    const double *A; int ns;                 // the tableau, ns columns
    double tau, tg;                          // the step and tau gamma
    double *xs, *mx, *fv, *y, **F;           // the state x, M x, f, the stage value (y_s: the new state) and F_j = f - K y_j
    const double *wg;                        // ext(g)
    bool from_guess;                         // the stage solves stop relative to the increment, not to the right-hand side
    double tol; int maxiter, check_every;
    bool keep_last_F;                        // F_s is formed too: F_1 of the next step, or weighed by the embedded rule
    int32_t *stage_iters;                    // ns of them: the iterations of every stage that was solved (the others: untouched)
    float *spmv_ms, *combine_ms, *solve_ms;  // the phase buckets of T
};

int dirk_stage_chain(hipStream_t st, igx_solver *s, const StageChain &c, PhaseTimer &T, bool &ok)
{
    const long long n = s->n;
    const unsigned nbv = vec_blocks(n), nbm = (unsigned)((n + 255) / 256);
    const int ns = c.ns;
    const double *A = c.A, *yprev = c.xs;
    ok = true;
    for (int i = 0; i < ns && ok; ++i) {
        const double aii = A[i * ns + i];
        if (aii == 0.0) continue;                                // (i = 0: y_1 = x, F_1 in F[0])
        Comb L{};
        L.c[L.nv] = 1.0; L.v[L.nv++] = c.mx;
        for (int j = 0; j < i; ++j)
            if (A[i * ns + j] != 0.0) { L.c[L.nv] = c.tau * A[i * ns + j]; L.v[L.nv++] = c.F[j]; }
        L.c[L.nv] = c.tg; L.v[L.nv++] = c.fv;
        k_dirk_rhs<<<nbv, BLOCK, 0, st>>>(n, L, s->b);
        k_mask_copy<<<nbm, 256, 0, st>>>(n, s->d_mask, yprev, s->x);    // the initial guess y_{i-1}
        IGX_HIP(hipGetLastError());
        if (int rc = T.lap(st, *c.combine_ms)) return rc;
        igx_solve_info si{};
        if (int rc = solve_lifted(st, s, c.wg, true, c.tol, c.maxiter, c.check_every, 0, si, c.from_guess)) return rc;
        if (int rc = T.lap(st, *c.solve_ms)) return rc;
        c.stage_iters[i] = si.iterations;
        if (!si.converged) { ok = false; break; }
        Comb Y{};
        Y.nv = 2; Y.c[0] = 1.0; Y.v[0] = s->x; Y.c[1] = 1.0; Y.v[1] = c.wg;        // y_i = x + ext(g)
        k_dirk_rhs<<<nbv, BLOCK, 0, st>>>(n, Y, c.y);
        IGX_HIP(hipGetLastError());
        if (int rc = T.lap(st, *c.combine_ms)) return rc;
        yprev = c.y;
        if (i < ns - 1 || c.keep_last_F) {                       // F_i = f - K y_i
            if (int rc = spmv_values(st, s, s->pv[1], c.y, c.fv, -1.0, c.F[i])) return rc;
            if (int rc = T.lap(st, *c.spmv_ms)) return rc;
        }
    }
    return IGX_OK;
}

} // namespace

extern "C" {

int igx_solver_create_parabolic(igx_patch *pt, int kind_K, int symmetric, const int64_t *fixed, int64_t nfixed, igx_solver **out)
{
    const char *what = "igx_solver_create_parabolic";
    if (!create_args_ok(pt, fixed, nfixed, out, what)) return IGX_ERR_ARG;
    if (kind_K != IGX_MASS && kind_K != IGX_STIFFNESS && kind_K != IGX_CONVDIFF && kind_K != IGX_FORM) {
        set_error("%s: unknown kind %d", what, kind_K);
        return IGX_ERR_ARG;
    }
    igx_solver *s = nullptr;
    if (int rc = create_patch_solver(pt, kind_K, 1, false, fixed, nfixed, &s, what)) return rc;
    s->parabolic = true;
    s->symmetric = symmetric != 0;
    if (!s->symmetric) {
        if (int rc = init_bicgstab(s, what)) { free_solver(s); return rc; }
        s->method = IGX_METHOD_BICGSTAB;
    }
    *out = s;
    return IGX_OK;
}

int igx_solver_take_values(igx_solver *s, int role)
{
    const char *what = "igx_solver_take_values";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    if (role != IGX_ROLE_MASS && role != IGX_ROLE_OPERATOR) { set_error("%s: unknown role %d", what, role); return IGX_ERR_ARG; }
    if (s->pv[role]) { set_error("%s: role %d was taken already", what, role); return IGX_ERR_ARG; }
    igx_patch *pt = s->pt;
    const int kind = role == IGX_ROLE_MASS ? IGX_MASS : s->kind;
    if (pt->values_kind != kind || !pt->d_data) {
        set_error("%s: the patch holds no values of kind %d: assemble them first (igx_assemble, data_out may be NULL)", what, kind);
        return IGX_ERR_ARG;
    }
    const int other = 1 - role;
    if (s->pv[other] && s->nvals[other] != pt->nnz) {
        set_error("%s: value buffers of unequal length (%lld and %lld)", what, (long long)pt->nnz, s->nvals[other]);
        return IGX_ERR_ARG;
    }
    IGX_HIP(hipSetDevice(s->ctx->device));
    IGX_HIP(hipStreamSynchronize(pt->ctx->stream));
    s->pv[role] = pt->d_data;                       // the buffer changes hands: the patch's next assembly allocates anew
    s->nvals[role] = pt->nnz;
    pt->d_data = nullptr;
    pt->values_kind = -1;
    return IGX_OK;
}

int igx_solver_set_dirk(igx_solver *s, int stages, const double *A, double tau)
{
    const char *what = "igx_solver_set_dirk";
    if (!s || !A) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    if (!s->pv[IGX_ROLE_MASS] || !s->pv[IGX_ROLE_OPERATOR]) { set_error("%s: take M and K first (igx_solver_take_values)", what); return IGX_ERR_ARG; }
    double gamma = 0.0;
    if (!dirk_ok(stages, A, tau, gamma, what)) return IGX_ERR_ARG;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (int rc = alloc_stage_matrix(s, what)) return rc;
    s->c_formed = false;
    s->precond = IGX_PRECOND_NONE;                   // (Jacobi's diagonal and the Kronecker factors depend on C: set them again)
    s->pc_vals = -1;
    if (int rc = form_stage_matrix(st, s, tau * gamma)) return rc;
    IGX_HIP(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&s->axpby_ms, s->dev[0], s->dev[1]);
    s->stages = stages;
    std::copy(A, A + (stages + 1) * stages, s->dirk_A);
    s->tau = tau;
    s->gamma = gamma;
    s->c_tg = tau * gamma;
    s->c_formed = true;
    return IGX_OK;
}

// Not built on the session calls (igx_solver_step_*), and dirk_A / tau / gamma not merged with st_*: the session scales the Kronecker
// eigenvalues on the device and stops its stage solves relative to the increment, so the iteration counts would change.
int igx_solver_dirk_run(igx_solver *s, const double *f, const double *gvals, const double *x0, int64_t nsteps, int64_t save_every,
                        double tol, int maxiter, int check_every, int timed, double *saved, int32_t *stage_iters, igx_dirk_info *info)
{
    const char *what = "igx_solver_dirk_run";
    if (!s || !f || (!gvals && !s->fixed.empty()) || !x0 || !saved) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    if (nsteps < 1 || save_every < 1) { set_error("%s: nsteps and save_every must be >= 1", what); return IGX_ERR_ARG; }
    if (!(tol >= 0.0) || maxiter < 0) { set_error("%s: tol must be >= 0 and maxiter >= 0", what); return IGX_ERR_ARG; }
    if (int rc = check_values(s, what)) return rc;
    if (s->c_tg != s->tau * s->gamma || s->pc_vals != -1) {
        set_error("%s: a stepping session (igx_solver_step_attempt) formed C or its preconditioner data since igx_solver_set_dirk: "
                  "set the tableau and the preconditioner again", what);
        return IGX_ERR_ARG;
    }
    if (check_every < 1) check_every = 1;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    if (int rc = alloc_dirk_vectors(s, what)) return rc;
    s->step_live = false;                                            // (the vectors of a stepping session are overwritten)
    double *xs = s->d_dirk, *mx = xs + n, *fv = xs + 2 * n, *y = xs + 3 * n, *F[IGX_DIRK_MAX_STAGES];
    for (int j = 0; j < IGX_DIRK_MAX_STAGES; ++j) F[j] = xs + (4 + j) * n;
    const int ns = s->stages;
    const double *A = s->dirk_A, tau = s->tau, gamma = s->gamma;
    const bool explicit_first = A[0] == 0.0;
    igx_dirk_info inf{};
    inf.axpby_ms = s->axpby_ms;
    s->breakdown = 0;
    hipEvent_t *E = s->dev;
    if (int rc = upload_start_state(st, s, f, gvals, x0, xs, s->w, fv, E[4])) return rc;      // ext(g) in s->w
    PhaseTimer T{E, 0, 1, timed};
    if (timed) IGX_HIP(hipEventRecord(E[0], st));
    auto save = [&]() -> int {                                      // the state xs to the next slot of `saved`
        IGX_HIP(hipMemcpyAsync(saved + (size_t)inf.nsaved * n, xs, nbytes, hipMemcpyDeviceToHost, st));
        IGX_HIP(hipStreamSynchronize(st));
        ++inf.nsaved;
        return IGX_OK;
    };
    if (explicit_first) {                                            // F_1 of the first step: f - K x0
        if (int rc = spmv_values(st, s, s->pv[1], xs, fv, -1.0, F[0])) return rc;
        if (int rc = T.lap(st, inf.spmv_ms)) return rc;
    }
    bool ok = true;
    long long last_saved = 0;
    for (long long k = 1; k <= nsteps && ok; ++k) {
        if (int rc = spmv_values(st, s, s->pv[0], xs, nullptr, 1.0, mx)) return rc;          // M x
        if (int rc = T.lap(st, inf.spmv_ms)) return rc;
        int32_t it[IGX_DIRK_MAX_STAGES];
        std::fill(it, it + ns, -1);                                  // (-1: not solved)
        // the stage solves stop relative to their right-hand side; the last F only as F_1 of the next step
        const StageChain chain{A, ns, tau, tau * gamma, xs, mx, fv, y, F, s->w, false, tol, maxiter, check_every, explicit_first,
                               it, &inf.spmv_ms, &inf.combine_ms, &inf.solve_ms};
        if (int rc = dirk_stage_chain(st, s, chain, T, ok)) return rc;
        for (int i = 0; i < ns; ++i) {
            if (it[i] < 0) continue;
            if (stage_iters) stage_iters[(k - 1) * ns + i] = it[i];
            inf.iterations += it[i];
            inf.max_stage_iterations = std::max(inf.max_stage_iterations, it[i]);
        }
        if (!ok) break;
        std::swap(xs, y);                                            // x_new = y_s
        if (explicit_first) std::swap(F[0], F[ns - 1]);
        inf.steps = k;
        if (k % save_every == 0 || k == nsteps) {
            if (int rc = save()) return rc;
            last_saved = k;
        }
    }
    if (!ok && inf.steps > 0 && last_saved != inf.steps) {          // the state after the last completed step
        if (int rc = save()) return rc;
    }
    if (int rc = close_call(st, E[4], E[5], what, inf.total_ms)) return rc;
    inf.converged = ok ? 1 : 0;
    if (info) *info = inf;
    return IGX_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// Adaptive steps and Rosenbrock methods: a session of attempts (pyiga/solvers.py:430-435, 475-534, 684-707).
// The host drives the controller; one attempt runs wholly on the device and leaves a candidate beside the untouched state.

namespace {

// a Rosenbrock scheme: A strictly lower triangular, Gamma lower triangular with one positive diagonal value (gamma out)
bool rosenbrock_ok(int st, const double *A, const double *G, const double *b, const double *bh, double &gamma, const char *what)
{
    if (st < 1 || st > IGX_DIRK_MAX_STAGES) { set_error("%s: %d stages (1 to %d)", what, st, IGX_DIRK_MAX_STAGES); return false; }
    for (int i = 0; i < st; ++i) {
        if (!std::isfinite(b[i]) || (bh && !std::isfinite(bh[i]))) { set_error("%s: a weight of stage %d is not finite", what, i); return false; }
        for (int j = 0; j < st; ++j) {
            const double a = A[i * st + j], g = G[i * st + j];
            if (!std::isfinite(a) || !std::isfinite(g)) { set_error("%s: entry [%d][%d] is not finite", what, i, j); return false; }
            if (j >= i && a != 0.0) { set_error("%s: A is not strictly lower triangular (A[%d][%d] = %g)", what, i, j, a); return false; }
            if (j > i && g != 0.0) { set_error("%s: Gamma is not lower triangular (Gamma[%d][%d] = %g)", what, i, j, g); return false; }
        }
    }
    gamma = G[0];
    if (!(gamma > 0.0)) { set_error("%s: the diagonal of Gamma must be positive (%g)", what, gamma); return false; }
    for (int i = 1; i < st; ++i)
        if (G[i * st + i] != gamma) {
            set_error("%s: two diagonal values of Gamma (%.17g and %.17g): C would change per stage", what, gamma, G[i * st + i]);
            return false;
        }
    return true;
}

// the preconditioner data of the session for the values `which` (0: M, 2: C with this tau gamma): the eigenvalue slots of the
// Kronecker factors (k_kron_lam) or Jacobi's diagonal (k_diag on the values in use); nothing if they are in place
int step_refresh_precond(hipStream_t st, igx_solver *s, int which, double tg)
{
    s->precond = s->step_precond;
    if (s->pc_vals == which && (which == 0 || s->pc_tg == tg)) return IGX_OK;
    if (s->step_precond == IGX_PRECOND_KRON) {
        k_kron_lam<<<1, 256, 0, st>>>(s->lam_slots, s->d_lamraw, s->d_kron, which == 0 ? 0.0 : tg, 1.0 / s->dim);
        IGX_HIP(hipGetLastError());
    } else if (s->step_precond == IGX_PRECOND_JACOBI) {
        k_diag<<<(unsigned)((s->n + 255) / 256), 256, 0, st>>>(s->g, patch_values(s), s->d_mask, s->dinv);
        IGX_HIP(hipGetLastError());
    }
    s->pc_vals = which;
    s->pc_tg = tg;
    return IGX_OK;
}

// sum over the free dofs of ((sum_k c_k v_k) / (tol + tol |x|))^2 into *sum (host), by k_err_norm and k_fin
int err_norm(hipStream_t st, igx_solver *s, const Comb &L, const double *x, double tol, double *sum)
{
    const unsigned nbv = vec_blocks(s->n);
    bool v2 = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (reinterpret_cast<uintptr_t>(s->d_mask) % 2 == 0);
    for (int k = 0; k < L.nv; ++k) v2 = v2 && reinterpret_cast<uintptr_t>(L.v[k]) % 16 == 0;
    if (v2) k_err_norm<true><<<nbv, BLOCK, 0, st>>>(s->n, L, x, s->d_mask, tol, s->d_part);
    else k_err_norm<false><<<nbv, BLOCK, 0, st>>>(s->n, L, x, s->d_mask, tol, s->d_part);
    k_fin<<<1, BLOCK, 0, st>>>(s->d_part, nullptr, nbv, s->d_sc, FIN_INIT);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipMemcpyAsync(sum, s->d_sc + SC_RR, sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

bool step_solver_ok(const igx_solver *s, const char *what)
{
    if (!s) { set_error("%s: null solver", what); return false; }
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return false; }
    if (!s->pv[IGX_ROLE_MASS] || !s->pv[IGX_ROLE_OPERATOR]) { set_error("%s: take M and K first (igx_solver_take_values)", what); return false; }
    return true;
}

} // namespace

extern "C" {

int igx_solver_set_stepper(igx_solver *s, int family, int stages, const double *A, const double *Gamma, const double *b,
                           const double *b_hat)
{
    const char *what = "igx_solver_set_stepper";
    if (!s || !A) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    double gamma = 0.0;
    if (family == IGX_STEPPER_DIRK) {
        if (Gamma) { set_error("%s: a DIRK scheme has no Gamma", what); return IGX_ERR_ARG; }
        if (!dirk_ok(stages, A, 1.0, gamma, what)) return IGX_ERR_ARG;
        for (int j = 0; j < stages; ++j) {
            if (b && b[j] != A[stages * stages + j]) { set_error("%s: b differs from the last row of A at %d", what, j); return IGX_ERR_ARG; }
            if (b_hat && !std::isfinite(b_hat[j])) { set_error("%s: b_hat[%d] is not finite", what, j); return IGX_ERR_ARG; }
        }
        std::copy(A, A + (stages + 1) * stages, s->st_A);
        std::copy(A + stages * stages, A + (stages + 1) * stages, s->st_b);
    } else if (family == IGX_STEPPER_ROSENBROCK) {
        if (!Gamma || !b) { set_error("%s: a Rosenbrock scheme needs Gamma and b", what); return IGX_ERR_ARG; }
        if (!rosenbrock_ok(stages, A, Gamma, b, b_hat, gamma, what)) return IGX_ERR_ARG;
        std::copy(A, A + stages * stages, s->st_A);
        std::copy(Gamma, Gamma + stages * stages, s->st_G);
        std::copy(b, b + stages, s->st_b);
    } else { set_error("%s: unknown family %d", what, family); return IGX_ERR_ARG; }
    s->st_bhat = b_hat != nullptr;
    if (b_hat) std::copy(b_hat, b_hat + stages, s->st_bh);
    s->family = family;
    s->st_stages = stages;
    s->st_gamma = gamma;
    s->step_live = false;                                 // (a session belongs to its scheme: begin again)
    return IGX_OK;
}

int igx_solver_set_step_precond(igx_solver *s, int precond, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                                const double *const *lam_raw)
{
    const char *what = "igx_solver_set_step_precond";
    if (!step_solver_ok(s, what)) return IGX_ERR_ARG;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    s->step_precond = -1;
    s->pc_vals = -1;
    if (precond == IGX_PRECOND_NONE || precond == IGX_PRECOND_JACOBI) { s->step_precond = precond; return IGX_OK; }
    if (precond != IGX_PRECOND_KRON) { set_error("%s: preconditioner %d (none, Jacobi or Kronecker)", what, precond); return IGX_ERR_ARG; }
    int nb[3];
    if (int rc = box_fastdiag_setup(s, 0, box_lo, box_hi, U, lam_raw, IGX_KRON_SUM, what, &s->precond, s->d_kron, nb)) return rc;
    if (int rc = alloc_fastdiag_work(s, (long long)nb[0] * nb[1] * nb[2])) return rc;
    std::vector<double> raw;
    LamSlots L{};
    L.nax = s->dim;
    size_t o = 0;
    for (int k = 0; k < s->dim; ++k) {                   // (the layout of pack_fastdiag: U_k^T | U_k | lam_k)
        const size_t mk = (size_t)nb[k];
        L.m[k] = nb[k];
        L.slot[k] = (long long)(o + 2 * mk * mk);
        L.raw[k] = (long long)raw.size();
        raw.insert(raw.end(), lam_raw[k], lam_raw[k] + mk);
        o += 2 * mk * mk + mk;
    }
    if (int rc = upload_replacing(st, raw, s->d_lamraw)) return rc;
    s->kron = box_fastdiag(s, 0, box_lo, nb, s->d_kron, IGX_KRON_SUM);
    s->lam_slots = L;
    IGX_HIP(hipStreamSynchronize(st));
    s->step_precond = IGX_PRECOND_KRON;
    return IGX_OK;
}

int igx_solver_step_begin(igx_solver *s, const double *f, const double *gvals, const double *x0)
{
    const char *what = "igx_solver_step_begin";
    if (!step_solver_ok(s, what)) return IGX_ERR_ARG;
    if (!f || (!gvals && !s->fixed.empty()) || !x0) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (s->family < 0) { set_error("%s: no scheme yet (igx_solver_set_stepper)", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    s->step_live = false;
    if (int rc = alloc_dirk_vectors(s, what)) return rc;
    if (int rc = alloc_stage_matrix(s, what)) return rc;
    if (!s->d_wg) {
        if (hipMalloc((void **)&s->d_wg, nbytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: out of device memory (%.3f GB)", what, nbytes / 1e9);
            return IGX_ERR_NOMEM;
        }
    }
    double *v = s->d_dirk;
    s->sx = v; s->smx = v + n; s->sfv = v + 2 * n; s->sy = v + 3 * n;
    for (int j = 0; j < IGX_DIRK_MAX_STAGES; ++j) s->sF[j] = v + (4 + j) * n;
    if (int rc = upload_start_state(st, s, f, gvals, x0, s->sx, s->d_wg, s->sfv, nullptr)) return rc;
    s->have_mx = s->have_F0 = s->have_cand = false;
    s->breakdown = 0;
    s->step_live = true;
    return IGX_OK;
}

int igx_solver_step_attempt(igx_solver *s, double tau, double err_tol, double solve_tol, int maxiter, int check_every, int timed,
                            igx_step_info *info)
{
    const char *what = "igx_solver_step_attempt";
    if (!step_solver_ok(s, what)) return IGX_ERR_ARG;
    if (!s->step_live) { set_error("%s: no session (igx_solver_step_begin; igx_solver_dirk_run and igx_solver_set_stepper end one)", what); return IGX_ERR_ARG; }
    if (s->step_precond < 0) { set_error("%s: no preconditioner of the session (igx_solver_set_step_precond; igx_solver_set_precond replaces it)", what); return IGX_ERR_ARG; }
    if (!(tau > 0.0) || !std::isfinite(tau)) { set_error("%s: tau must be positive and finite", what); return IGX_ERR_ARG; }
    if (!(solve_tol >= 0.0) || maxiter < 0) { set_error("%s: solve_tol must be >= 0 and maxiter >= 0", what); return IGX_ERR_ARG; }
    if (err_tol > 0.0 && !s->st_bhat) { set_error("%s: the scheme has no embedded rule (b_hat): err_tol must be <= 0", what); return IGX_ERR_ARG; }
    if (check_every < 1) check_every = 1;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const long long n = s->n;
    const int ns = s->st_stages;
    const double *A = s->st_A, gamma = s->st_gamma, tg = tau * gamma;
    const bool estimate = err_tol > 0.0;
    const unsigned nbv = vec_blocks(n);
    igx_step_info inf{};
    inf.n_free = n - (long long)s->fixed.size();
    inf.has_estimate = estimate ? 1 : 0;
    s->have_cand = false;
    s->breakdown = 0;
    s->vals_sel = nullptr;
    hipEvent_t *E = s->dev;
    IGX_HIP(hipEventRecord(E[4], st));
    if (!s->c_formed || s->c_tg != tg) {                            // C on the device belongs to another step
        s->c_formed = false;
        if (int rc = form_stage_matrix(st, s, tg)) return rc;
        IGX_HIP(hipEventSynchronize(E[1]));
        (void)hipEventElapsedTime(&s->axpby_ms, E[0], E[1]);
        inf.axpby_ms = s->axpby_ms;
        inf.reformed = 1;
        s->c_tg = tg;
        s->c_formed = true;
        s->pc_vals = -1;
    }
    if (int rc = step_refresh_precond(st, s, 2, tg)) return rc;
    PhaseTimer T{E, 2, 3, timed};                                    // (E[0], E[1]: k_vals_axpby)
    if (timed) IGX_HIP(hipEventRecord(E[2], st));
    bool ok = true;
    double sum = 0.0;
    if (s->family == IGX_STEPPER_DIRK) {
        double *xs = s->sx, *mx = s->smx, *fv = s->sfv, *y = s->sy, **F = s->sF;
        const bool explicit_first = A[0] == 0.0;
        if (explicit_first && !s->have_F0) {                         // F_1 of the first step: f - K x0
            if (int rc = spmv_values(st, s, s->pv[1], xs, fv, -1.0, F[0])) return rc;
            s->have_F0 = true;
        }
        if (!s->have_mx) {                                           // M x: kept over rejected attempts
            if (int rc = spmv_values(st, s, s->pv[0], xs, nullptr, 1.0, mx)) return rc;
            s->have_mx = true;
        }
        if (int rc = T.lap(st, inf.spmv_ms)) return rc;
        // the stage solves stop relative to the increment; the last F as F_1 of the next step, or where the embedded rule weighs it
        const bool have_Fs = explicit_first || (estimate && s->st_bh[ns - 1] != s->st_b[ns - 1]);
        const StageChain chain{A, ns, tau, tg, xs, mx, fv, y, F, s->d_wg, true, solve_tol, maxiter, check_every, have_Fs,
                               inf.stage_iterations, &inf.spmv_ms, &inf.combine_ms, &inf.solve_ms};
        if (int rc = dirk_stage_chain(st, s, chain, T, ok)) return rc;
        if (ok && estimate) {
            // e = x_est - x_new: the last stage equation is M x_new = M x + tau sum b_i F_i, so R M R^T e = tau sum (b^_i - b_i) F_i
            // (the F_i vanish on the fixed dofs; nothing to lift).  One CG solve on M from zero: its relative residual is that
            // of the estimate itself, not of the 1/err_tol times larger x_est
            Comb L{};
            for (int j = 0; j < ns; ++j) {
                const double c = s->st_bh[j] - s->st_b[j];
                if (c != 0.0 && (j < ns - 1 || have_Fs)) { L.c[L.nv] = tau * c; L.v[L.nv++] = F[j]; }
            }
            k_dirk_rhs<<<nbv, BLOCK, 0, st>>>(n, L, s->b);
            IGX_HIP(hipGetLastError());
            if (int rc = T.lap(st, inf.combine_ms)) return rc;
            s->vals_sel = s->pv[IGX_ROLE_MASS];
            const int method = s->method;
            s->method = IGX_METHOD_CG;                               // (M is symmetric positive definite whatever K is)
            igx_solve_info si{};
            int rc = step_refresh_precond(st, s, 0, 0.0);
            if (!rc) rc = solve_lifted(st, s, nullptr, false, solve_tol, maxiter, check_every, 0, si);
            s->method = method;
            s->vals_sel = nullptr;
            if (rc) return rc;
            if (int rc2 = T.lap(st, inf.mass_ms)) return rc2;
            inf.mass_iterations = si.iterations;
            if (!si.converged) ok = false;
            else {
                Comb D{};
                D.nv = 1; D.c[0] = 1.0; D.v[0] = s->x;
                if (int rc2 = err_norm(st, s, D, xs, err_tol, &sum)) return rc2;
                if (int rc2 = T.lap(st, inf.err_ms)) return rc2;
            }
        }
    } else {
        // Rosenbrock: C k_i = f~ - K (x + tau sum_j (a_ij + gamma_ij) k_j) on the free dofs, k_i = 0 on the fixed ones
        double *xs = s->sx, *cand = s->smx, *fv = s->sfv, *yt = s->sy, **K = s->sF;
        const double *G = s->st_G;
        for (int i = 0; i < ns && ok; ++i) {
            Comb L{};
            L.c[L.nv] = 1.0; L.v[L.nv++] = xs;
            for (int j = 0; j < i; ++j) {
                const double c = A[i * ns + j] + G[i * ns + j];
                if (c != 0.0) { L.c[L.nv] = tau * c; L.v[L.nv++] = K[j]; }
            }
            const double *yi = xs;
            if (L.nv > 1) {
                k_dirk_rhs<<<nbv, BLOCK, 0, st>>>(n, L, yt);
                IGX_HIP(hipGetLastError());
                if (int rc = T.lap(st, inf.combine_ms)) return rc;
                yi = yt;
            }
            if (int rc = spmv_values(st, s, s->pv[1], yi, fv, -1.0, s->b)) return rc;
            if (int rc = T.lap(st, inf.spmv_ms)) return rc;
            igx_solve_info si{};
            if (int rc = solve_lifted(st, s, nullptr, false, solve_tol, maxiter, check_every, 0, si)) return rc;
            IGX_HIP(hipMemcpyAsync(K[i], s->x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (int rc = T.lap(st, inf.solve_ms)) return rc;
            inf.stage_iterations[i] = si.iterations;
            if (!si.converged) ok = false;
        }
        if (ok) {
            Comb L{};
            L.c[L.nv] = 1.0; L.v[L.nv++] = xs;
            for (int j = 0; j < ns; ++j)
                if (s->st_b[j] != 0.0) { L.c[L.nv] = tau * s->st_b[j]; L.v[L.nv++] = K[j]; }
            k_dirk_rhs<<<nbv, BLOCK, 0, st>>>(n, L, cand);
            IGX_HIP(hipGetLastError());
            if (int rc = T.lap(st, inf.combine_ms)) return rc;
            if (estimate) {
                Comb D{};
                for (int j = 0; j < ns; ++j) {
                    const double c = s->st_bh[j] - s->st_b[j];
                    if (c != 0.0) { D.c[D.nv] = tau * c; D.v[D.nv++] = K[j]; }
                }
                if (int rc = err_norm(st, s, D, xs, err_tol, &sum)) return rc;
                if (int rc = T.lap(st, inf.err_ms)) return rc;
            }
        }
    }
    if (int rc = close_call(st, E[4], E[5], what, inf.total_ms)) return rc;
    inf.converged = ok ? 1 : 0;
    inf.r = (ok && estimate) ? std::sqrt(sum) / std::sqrt((double)std::max<long long>(1, inf.n_free)) : 0.0;
    s->have_cand = ok;
    if (info) *info = inf;
    return IGX_OK;
}

int igx_solver_step_accept(igx_solver *s)
{
    const char *what = "igx_solver_step_accept";
    if (!step_solver_ok(s, what)) return IGX_ERR_ARG;
    if (!s->step_live || !s->have_cand) { set_error("%s: no candidate (a converged igx_solver_step_attempt first)", what); return IGX_ERR_ARG; }
    if (s->family == IGX_STEPPER_DIRK) {
        std::swap(s->sx, s->sy);                                     // x_new = y_s
        if (s->st_A[0] == 0.0) std::swap(s->sF[0], s->sF[s->st_stages - 1]);
    } else std::swap(s->sx, s->smx);
    s->have_mx = false;
    s->have_cand = false;
    return IGX_OK;
}

int igx_solver_step_state(igx_solver *s, int which, double *out)
{
    const char *what = "igx_solver_step_state";
    if (!step_solver_ok(s, what)) return IGX_ERR_ARG;
    if (!out) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->step_live) { set_error("%s: no session (igx_solver_step_begin)", what); return IGX_ERR_ARG; }
    if (which != IGX_STEP_STATE && which != IGX_STEP_CANDIDATE) { set_error("%s: unknown vector %d", what, which); return IGX_ERR_ARG; }
    if (which == IGX_STEP_CANDIDATE && !s->have_cand) { set_error("%s: no candidate (a converged igx_solver_step_attempt first)", what); return IGX_ERR_ARG; }
    const double *src = which == IGX_STEP_STATE ? s->sx : s->family == IGX_STEPPER_DIRK ? s->sy : s->smx;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipMemcpyAsync(out, src, (size_t)s->n * sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_solver_error_ratio_d(igx_solver *s, int nv, const double *coef, const double *const *d_v, const double *d_x, double tol,
                             double *r)
{
    const char *what = "igx_solver_error_ratio_d";
    if (!s || !coef || !d_v || !d_x || !r) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (nv < 1 || nv > COMB_MAX) { set_error("%s: %d vectors (1 to %d)", what, nv, COMB_MAX); return IGX_ERR_ARG; }
    if (!(tol > 0.0)) { set_error("%s: tol must be positive", what); return IGX_ERR_ARG; }
    Comb L{};
    for (int k = 0; k < nv; ++k) {
        if (!d_v[k]) { set_error("%s: vector %d is null", what, k); return IGX_ERR_ARG; }
        L.c[k] = coef[k]; L.v[k] = d_v[k];
    }
    L.nv = nv;
    IGX_HIP(hipSetDevice(s->ctx->device));
    double sum = 0.0;
    if (int rc = err_norm(s->ctx->stream, s, L, d_x, tol, &sum)) return rc;
    const long long nfree = s->n - (long long)s->fixed.size();
    *r = std::sqrt(sum) / std::sqrt((double)std::max<long long>(1, nfree));
    return IGX_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// Block kernels of the eigen-solver (igx_solver_eig_*).  A block holds MB interleaved columns: entry (I, j)
// at I * MB + j, MB = 4, 8 or 16; padding columns are zero.
namespace {

// The sum over the GW lanes of a group of T = 2^t values per lane as a reduce-scatter: at every shuffle step a lane keeps one
// half of its values and adds the other lane's copies of that half, so T - 1 shuffle-adds (while more than one value is left)
// instead of T log2(GW).  With T >= GW lane l ends with the T / GW sums of the original indices base .. base + T / GW - 1 in
// a[0 ..]; with T < GW the steps left over are a butterfly on the one value, and the lanes with (l & (GW / T - 1)) == 0 hold
// distinct sums.  The order of the additions is fixed.
template <int GW, int OFF, int T>
struct ReduceScatter {
    static __device__ __forceinline__ void run(double *a, int lane, int &base)
    {
        if constexpr (OFF > 0) {
            if constexpr (T > 1) {
                constexpr int H = T / 2;
                const bool up = (lane & OFF) != 0;
#pragma unroll
                for (int i = 0; i < H; ++i) {
                    const double send = up ? a[i] : a[i + H], keep = up ? a[i + H] : a[i];
                    a[i] = keep + __shfl_xor(send, OFF, GW);
                }
                if (up) base += H;
                ReduceScatter<GW, OFF / 2, H>::run(a, lane, base);
            } else {
                a[0] += __shfl_xor(a[0], OFF, GW);
                ReduceScatter<GW, OFF / 2, 1>::run(a, lane, base);
            }
        }
    }
};

// The block product, the hot kernel: yK = mask . K . x and (NM == 2) yM = mask . M . x for a block x of MB columns in one pass
// over the structured layout.  The row-to-group map, the row header one row ahead and the lane's walk through the row are
// k_spmv's.  Per entry a lane loads its K value and its M value once (non-temporal: they are not read again by this pass) and the
// MB contiguous x-entries of that column as 16-byte loads, and keeps NM MB sums: the value arrays are read once per block, not
// once per column, and the x-gather is shared by the two matrices.  U entries of a lane are in flight before they are summed.
// x must vanish on the fixed dofs (R^T); the rows of fixed dofs are not read and come out as 0.
template <int GW, int MB, int U, int NM>
__global__ void __launch_bounds__(BLOCK) k_spmm2(const Geom g, const double *__restrict__ vK, const double *__restrict__ vM,
                                                 const uint8_t *__restrict__ freem, const double *__restrict__ x,
                                                 double *__restrict__ yK, double *__restrict__ yM)
{
    constexpr int T = NM * MB, H = MB / 2;
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    const int N1 = g.N[1], N2 = g.N[2];
    const int N12 = N1 * N2;
    const dbl2 zero2 = {0.0, 0.0};
    long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW;
    RowHdr h{};
    if (I < g.nrows) h = row_hdr(g, freem, I);
    for (; I < g.nrows; I += ngroups) {
        const RowHdr cur = h;
        if (I + ngroups < g.nrows) h = row_hdr(g, freem, I + ngroups);
        if (!cur.fr) {                               // (uniform over the group)
            for (int j = lane; j < MB; j += GW) {
                yK[I * MB + j] = 0.0;
                if (NM == 2) yM[I * MB + j] = 0.0;
            }
            continue;
        }
        const int c0 = cur.c0 - cur.l0, c1 = cur.c1 - cur.l1, c2 = cur.c2 - cur.l2;
        const int len = c0 * c1 * c2;
        const long long row = igx_rowptr3(&cur.r0, &cur.r1, &cur.r2, g.S1, g.S2, c0, c1, 0, 0, 0);
        const int xbase = (cur.l0 * N1 + cur.l1) * N2 + cur.l2;
        int c = lane % c2, bb = (lane / c2) % c1, a = lane / (c1 * c2);
        const int dc = GW % c2, db = (GW / c2) % c1, da = GW / (c1 * c2);
        double acc[T];
#pragma unroll
        for (int i = 0; i < T; ++i) acc[i] = 0.0;
        for (int k0 = lane; k0 < len; k0 += U * GW) {
            double v[U][NM];
            dbl2 xv[U][H];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k0 + u * GW < len;
                v[u][0] = in ? __builtin_nontemporal_load(vK + row + k0 + u * GW) : 0.0;
                if (NM == 2) v[u][NM - 1] = in ? __builtin_nontemporal_load(vM + row + k0 + u * GW) : 0.0;
                const dbl2 *xr = reinterpret_cast<const dbl2 *>(x + (long long)(xbase + a * N12 + bb * N2 + c) * MB);
#pragma unroll
                for (int j = 0; j < H; ++j) xv[u][j] = in ? xr[j] : zero2;
                c += dc; bb += db; a += da;
                if (c >= c2) { c -= c2; ++bb; }
                if (bb >= c1) { bb -= c1; ++a; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < NM; ++q)
#pragma unroll
                    for (int j = 0; j < H; ++j) {
                        acc[q * MB + 2 * j] += v[u][q] * xv[u][j].x;
                        acc[q * MB + 2 * j + 1] += v[u][q] * xv[u][j].y;
                    }
        }
        int base = 0;
        ReduceScatter<GW, GW / 2, T>::run(acc, lane, base);
        constexpr int TF = T >= GW ? T / GW : 1;     // sums a writing lane holds: the original indices base .. base + TF - 1
        if (T >= GW || (lane & (GW / T - 1)) == 0) {
#pragma unroll
            for (int i = 0; i < TF; ++i) {
                const int o = base + i;              // (q, j) = (o / MB, o % MB); TF divides MB: one q per lane
                double *y = (NM == 2 && o >= MB) ? yM : yK;
                y[I * MB + (o % MB)] = acc[i];
            }
        }
    }
}

// f(the instantiation of the block product at group width gw) for a row stride MB and NM matrices: with with_spmm2_kernel the
// only place that names one (U: 32 / MB entries of a lane in flight at 64 lanes, 16 / MB below)
template <int MB, int NM, class F>
decltype(auto) with_spmm2_gw(int gw, F &&f)
{
    switch (gw) {
    case 64: return f(k_spmm2<64, MB, 32 / MB, NM>);
    case 32: return f(k_spmm2<32, MB, 16 / MB, NM>);
    case 16: return f(k_spmm2<16, MB, 16 / MB, NM>);
    case 8: return f(k_spmm2<8, MB, 16 / MB, NM>);
    default: return f(k_spmm2<4, MB, 16 / MB, NM>);
    }
}

template <class F>
decltype(auto) with_spmm2_kernel(int gw, int mb, int nm, F &&f)
{
    if (nm == 2) {
        switch (mb) {
        case 4: return with_spmm2_gw<4, 2>(gw, f);
        case 8: return with_spmm2_gw<8, 2>(gw, f);
        default: return with_spmm2_gw<16, 2>(gw, f);
        }
    }
    switch (mb) {
    case 4: return with_spmm2_gw<4, 1>(gw, f);
    case 8: return with_spmm2_gw<8, 1>(gw, f);
    default: return with_spmm2_gw<16, 1>(gw, f);
    }
}

// The block product over the general CSR pattern of a multipatch: k_spmm2's contract and inner structure,
// with k_csr_spmv's row-to-group map, its header (free flag, indptr) one row ahead and its 64-bit offsets.  Per entry a lane loads
// the K value, the M value and the column index once (non-temporal) and gathers the MB x-entries of that column as 16-byte loads.
// x must vanish on the fixed dofs; the rows of fixed dofs are not read and come out as 0.  Fixed order, no atomics.
template <int GW, int MB, int U, int NM>
__global__ void __launch_bounds__(BLOCK) k_csr_spmm2(long long nrows, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                     const double *__restrict__ vK, const double *__restrict__ vM,
                                                     const uint8_t *__restrict__ freem, const double *__restrict__ x,
                                                     double *__restrict__ yK, double *__restrict__ yM)
{
    constexpr int T = NM * MB, H = MB / 2;
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    const dbl2 zero2 = {0.0, 0.0};
    long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW;
    long long nk0 = 0, nk1 = 0;
    int nfr = 0;
    if (I < nrows) { nfr = freem[I]; nk0 = indptr[I]; nk1 = indptr[I + 1]; }
    for (; I < nrows; I += ngroups) {
        const long long k0 = nk0, k1 = nk1;
        const int fr = nfr;
        if (I + ngroups < nrows) { nfr = freem[I + ngroups]; nk0 = indptr[I + ngroups]; nk1 = indptr[I + ngroups + 1]; }
        if (!fr) {                                   // (uniform over the group)
            for (int j = lane; j < MB; j += GW) {
                yK[I * MB + j] = 0.0;
                if (NM == 2) yM[I * MB + j] = 0.0;
            }
            continue;
        }
        double acc[T];
#pragma unroll
        for (int i = 0; i < T; ++i) acc[i] = 0.0;
        for (long long k = k0 + lane; k < k1; k += U * GW) {
            double v[U][NM];
            int c[U];
            dbl2 xv[U][H];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k + u * GW < k1;
                v[u][0] = in ? __builtin_nontemporal_load(vK + k + u * GW) : 0.0;
                if (NM == 2) v[u][NM - 1] = in ? __builtin_nontemporal_load(vM + k + u * GW) : 0.0;
                c[u] = in ? __builtin_nontemporal_load(indices + k + u * GW) : -1;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const dbl2 *xr = reinterpret_cast<const dbl2 *>(x + (long long)(c[u] >= 0 ? c[u] : 0) * MB);
#pragma unroll
                for (int j = 0; j < H; ++j) xv[u][j] = c[u] >= 0 ? xr[j] : zero2;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < NM; ++q)
#pragma unroll
                    for (int j = 0; j < H; ++j) {
                        acc[q * MB + 2 * j] += v[u][q] * xv[u][j].x;
                        acc[q * MB + 2 * j + 1] += v[u][q] * xv[u][j].y;
                    }
        }
        int base = 0;
        ReduceScatter<GW, GW / 2, T>::run(acc, lane, base);
        constexpr int TF = T >= GW ? T / GW : 1;     // sums a writing lane holds: the original indices base .. base + TF - 1
        if (T >= GW || (lane & (GW / T - 1)) == 0) {
#pragma unroll
            for (int i = 0; i < TF; ++i) {
                const int o = base + i;              // (q, j) = (o / MB, o % MB); TF divides MB: one q per lane
                double *y = (NM == 2 && o >= MB) ? yM : yK;
                y[I * MB + (o % MB)] = acc[i];
            }
        }
    }
}

// the instantiations of the CSR block product, as with_spmm2_gw / with_spmm2_kernel name those of the structured one (U: the table
// of DESIGN.md section 23)
template <int MB, int NM, class F>
decltype(auto) with_csr_spmm2_gw(int gw, F &&f)
{
    switch (gw) {
    case 64: return f(k_csr_spmm2<64, MB, 32 / MB, NM>);
    case 32: return f(k_csr_spmm2<32, MB, 16 / MB, NM>);
    case 16: return f(k_csr_spmm2<16, MB, 16 / MB, NM>);
    case 8: return f(k_csr_spmm2<8, MB, 16 / MB, NM>);
    default: return f(k_csr_spmm2<4, MB, 16 / MB, NM>);
    }
}

template <class F>
decltype(auto) with_csr_spmm2_kernel(int gw, int mb, int nm, F &&f)
{
    if (nm == 2) {
        switch (mb) {
        case 4: return with_csr_spmm2_gw<4, 2>(gw, f);
        case 8: return with_csr_spmm2_gw<8, 2>(gw, f);
        default: return with_csr_spmm2_gw<16, 2>(gw, f);
        }
    }
    switch (mb) {
    case 4: return with_csr_spmm2_gw<4, 1>(gw, f);
    case 8: return with_csr_spmm2_gw<8, 1>(gw, f);
    default: return with_csr_spmm2_gw<16, 1>(gw, f);
    }
}

// column j of a block of mb interleaved columns as a contiguous vector (zero on the fixed dofs), and back: the V-cycle of a
// multipatch solver works on one vector, so a block goes through it column by column
__global__ void k_block_col_get(long long n, int mb, int j, const uint8_t *__restrict__ freem, const double *__restrict__ blk,
                                double *__restrict__ v)
{
    for (long long I = (long long)blockIdx.x * blockDim.x + threadIdx.x; I < n; I += (long long)gridDim.x * blockDim.x)
        v[I] = freem[I] ? blk[I * mb + j] : 0.0;
}

__global__ void k_block_col_put(long long n, int mb, int j, const double *__restrict__ v, double *__restrict__ blk)
{
    for (long long I = (long long)blockIdx.x * blockDim.x + threadIdx.x; I < n; I += (long long)gridDim.x * blockDim.x)
        blk[I * mb + j] = v[I];
}

// Gram matrix of up to three A blocks against up to three B blocks over the free rows, first stage: block `blockIdx.x` sums its
// chunks of GR_RC rows (chunk ch = blockIdx.x, + gridDim.x, ..: a fixed order) through LDS tiles; thread (ty, tx) keeps the
// entries (ty + 16 r, tx + 16 c) of the concatenated (3 MB) x (3 MB) matrix.  part[block][GR_W][GR_W], GR_W = 16 ceil(3 MB / 16).
constexpr int GR_RC = 32;
constexpr int NB_GRAM = 256;
struct GramArgs {
    const double *A[3], *B[3];
    int na, nb;
};

template <int MB>
__global__ void __launch_bounds__(BLOCK) k_gram(long long n, const GramArgs P, const uint8_t *__restrict__ freem, double *part)
{
    constexpr int R = (3 * MB + 15) / 16, GW_ = 16 * R;
    __shared__ double As[GR_RC][GW_ + 1], Bs[GR_RC][GW_ + 1];
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const int wa = P.na * MB, wb = P.nb * MB;
    double acc[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < R; ++c) acc[r][c] = 0.0;
    const long long nchunk = (n + GR_RC - 1) / GR_RC;
    for (long long ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        const long long I0 = ch * GR_RC;
        for (int e = t; e < GR_RC * GW_; e += BLOCK) {
            const int r = e / GW_, col = e % GW_;
            const long long I = I0 + r;
            const bool row_in = I < n && freem[I] != 0;
            const int b = col / MB, j = col % MB;
            const double *pa = b == 0 ? P.A[0] : b == 1 ? P.A[1] : P.A[2];
            const double *pb = b == 0 ? P.B[0] : b == 1 ? P.B[1] : P.B[2];
            As[r][col] = (row_in && col < wa) ? pa[I * MB + j] : 0.0;
            Bs[r][col] = (row_in && col < wb) ? pb[I * MB + j] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < GR_RC; ++k) {
            double av[R], bv[R];
#pragma unroll
            for (int r = 0; r < R; ++r) av[r] = As[k][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < R; ++c) bv[c] = Bs[k][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < R; ++c) acc[r][c] += av[r] * bv[c];
        }
        __syncthreads();
    }
    double *out = part + (long long)blockIdx.x * GW_ * GW_;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < R; ++c) out[(ty + 16 * r) * GW_ + tx + 16 * c] = acc[r][c];
}

// second stage: G[(ia m + a)][(ib m + b)] = the sum over the blocks, in their order, of part[block][ia MB + a][ib MB + b]
__global__ void k_gram_fin(const double *__restrict__ part, int nblocks, int gw, int mb, int m, int na, int nb, double *G)
{
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    const int rows = na * m, cols = nb * m;
    if (o >= rows * cols) return;
    const int ra = o / cols, cb = o % cols;
    const int pr = (ra / m) * mb + ra % m, pc = (cb / m) * mb + cb % m;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < nblocks; ++k) s += part[((long long)k * gw + pr) * gw + pc];     // (loads ahead of the adds; their order stays)
    G[o] = s;
}

// Block combinations: for every job z = blockIdx.y the block Y[z] = sum_{j < nsrc[z]} S[z][j] . C[coef[z] + j], the MB x MB
// coefficient blocks (row-major, zero-padded) read from `coef` at uniform addresses.  One thread per row.  No Y is a source.
constexpr int COMB_JOBS = 6;
struct BlockComb {
    const double *S[COMB_JOBS][3];
    double *Y[COMB_JOBS];
    int nsrc[COMB_JOBS], coef[COMB_JOBS];
};

template <int MB>
__global__ void __launch_bounds__(BLOCK) k_block_comb(long long n, const BlockComb P, const double *__restrict__ coef)
{
    const int z = blockIdx.y;
    const int ns = P.nsrc[z];
    const double *Cz = coef + (long long)P.coef[z] * MB * MB;
    for (long long I = (long long)blockIdx.x * BLOCK + threadIdx.x; I < n; I += (long long)gridDim.x * BLOCK) {
        double y[MB];
#pragma unroll
        for (int b = 0; b < MB; ++b) y[b] = 0.0;
        for (int j = 0; j < ns; ++j) {
            const dbl2 *sr = reinterpret_cast<const dbl2 *>(P.S[z][j] + I * MB);
            const double *Cj = Cz + j * MB * MB;
            dbl2 s[MB / 2];
#pragma unroll
            for (int a = 0; a < MB / 2; ++a) s[a] = sr[a];
#pragma unroll
            for (int a = 0; a < MB / 2; ++a)
#pragma unroll
                for (int b = 0; b < MB; ++b) {
                    y[b] += s[a].x * Cj[2 * a * MB + b];
                    y[b] += s[a].y * Cj[(2 * a + 1) * MB + b];
                }
        }
        dbl2 *yr = reinterpret_cast<dbl2 *>(P.Y[z] + I * MB);
#pragma unroll
        for (int b = 0; b < MB / 2; ++b) { const dbl2 v = {y[2 * b], y[2 * b + 1]}; yr[b] = v; }
    }
}

// the sums of a thread's values per column j = threadIdx.x % MB over the block, in sh[0 .. MB) (a fixed tree)
template <int MB>
__device__ __forceinline__ double col_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = BLOCK / 2; off >= MB; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    const double s = sh[threadIdx.x % MB];
    __syncthreads();
    return s;
}

// R = free ? KX - MX diag(lam) : 0 and the partial sums of R^2 and KX^2 per column over the free rows:
// part[(block * 2 + q) * MB + j].  The grid stride is a multiple of MB, so a thread stays in column threadIdx.x % MB.
template <int MB>
__global__ void __launch_bounds__(BLOCK) k_resid(long long n, const double *__restrict__ KX, const double *__restrict__ MX,
                                                 const double *__restrict__ lam, const uint8_t *__restrict__ freem, double *R,
                                                 double *part)
{
    __shared__ double sh[BLOCK];
    const int j = threadIdx.x % MB;
    const double l = lam[j];
    double sr = 0.0, sk = 0.0;
    const long long tot = n * MB;
    for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < tot; e += (long long)gridDim.x * BLOCK) {
        const bool fr = freem[e / MB] != 0;
        const double kx = fr ? KX[e] : 0.0, r = fr ? kx - l * MX[e] : 0.0;
        R[e] = r;
        sr += r * r;
        sk += kx * kx;
    }
    sr = col_sum<MB>(sr, sh);
    sk = col_sum<MB>(sk, sh);
    if ((int)threadIdx.x < MB) {
        part[((long long)blockIdx.x * 2 + 0) * MB + j] = sr;
        part[((long long)blockIdx.x * 2 + 1) * MB + j] = sk;
    }
}

// out[q * mb + j] = the sum over the blocks, in their order, of part[(block * 2 + q) * mb + j]
__global__ void k_col_fin(const double *__restrict__ part, int nblocks, int mb, double *out)
{
    const int o = threadIdx.x;
    if (o >= 2 * mb) return;
    const int q = o / mb, j = o % mb;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < nblocks; ++k) s += part[((long long)k * 2 + q) * mb + j];
    out[o] = s;
}

// y = free ? (d ? d[I] : 1) x : 0 on a block of mb columns: batched Jacobi scaling, or the masked copy
__global__ void k_block_scale(long long n, int mb, const double *__restrict__ d, const uint8_t *__restrict__ freem,
                              const double *__restrict__ x, double *__restrict__ y)
{
    const long long tot = n * mb;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
        const long long I = e / mb;
        y[e] = freem[I] ? (d ? d[I] * x[e] : x[e]) : 0.0;
    }
}

// ---- host side
bool eig_mb_ok(int mb) { return mb == 4 || mb == 8 || mb == 16; }
int eig_mb_slot(int mb) { return mb == 4 ? 0 : mb == 8 ? 1 : 2; }

int eig_check(const igx_solver *s, const char *what, bool values)
{
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (s->mp) {                              // K: the multipatch's current sums, M: the solver's own array
        if (!s->d_mass) { set_error("%s: a multipatch solver needs its mass matrix first (igx_solver_set_mass_d)", what); return IGX_ERR_ARG; }
        return values ? check_values(s, what) : IGX_OK;
    }
    if (!s->parabolic || !s->symmetric || s->ncomp != 1) {
        set_error("%s: needs a symmetric parabolic solver (igx_solver_create_parabolic) or a multipatch solver with a mass matrix "
                  "(igx_solver_set_mass_d)", what);
        return IGX_ERR_ARG;
    }
    if (!s->pv[IGX_ROLE_MASS] || !s->pv[IGX_ROLE_OPERATOR]) { set_error("%s: take M and K first (igx_solver_take_values)", what); return IGX_ERR_ARG; }
    return IGX_OK;
}

constexpr size_t EIG_SMALL = 4096;       // doubles of d_small: Gram result (<= 48 x 48) | coefficients at EIG_COEF | lam, norms at EIG_LAM
constexpr size_t EIG_COEF = 2304, EIG_LAM = EIG_COEF + 6 * 256, EIG_NORM = EIG_LAM + 16;

// the state of the eigen pieces (made once per solver): partial sums, the small buffer, the masked-input block, events
int eig_state(igx_solver *s, const char *what, EigState **out, bool values = true)
{
    if (int rc = eig_check(s, what, values)) return rc;
    IGX_HIP(hipSetDevice(s->ctx->device));
    if (!s->eig) {
        EigState *e = new EigState;
        const size_t gpart = (size_t)NB_GRAM * 48 * 48, cpart = (size_t)NB_VEC * 2 * EIG_MB_MAX;
        bool ok = hipMalloc((void **)&e->d_gpart, std::max(gpart, cpart) * sizeof(double)) == hipSuccess &&
                  hipMalloc((void **)&e->d_small, EIG_SMALL * sizeof(double)) == hipSuccess &&
                  hipMalloc((void **)&e->d_tmp, (size_t)s->n * EIG_MB_MAX * sizeof(double)) == hipSuccess;
        for (auto &ev : e->ev) ok = ok && hipEventCreate(&ev) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipFree(e->d_gpart); (void)hipFree(e->d_small); (void)hipFree(e->d_tmp);
            delete e;
            set_error("%s: out of device memory", what);
            return IGX_ERR_NOMEM;
        }
        e->have_ev = true;
        s->eig = e;
    }
    *out = s->eig;
    return IGX_OK;
}

int eig_session(igx_solver *s, const char *what, EigState **out)
{
    if (int rc = eig_state(s, what, out)) return rc;
    if (!(*out)->mb) { set_error("%s: no session (igx_solver_eig_begin)", what); return IGX_ERR_ARG; }
    return IGX_OK;
}

bool eig_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// phases of igx_eig_info
enum { PH_PRODUCTS = 0, PH_GRAM, PH_COMBINE, PH_RESID, PH_PRECOND };

struct EigPhase {                                    // events around a phase of a timed session
    hipStream_t st; EigState *e; int ph; bool on;
    EigPhase(hipStream_t st_, EigState *e_, int ph_, bool session) : st(st_), e(e_), ph(ph_), on(session && e_->timed)
    {
        if (on) (void)hipEventRecord(e->ev[0], st);
    }
    int done()
    {
        int32_t *cnt[] = {&e->info.products, &e->info.grams, &e->info.combines, &e->info.residuals, &e->info.preconds};
        float *ms[] = {&e->info.products_ms, &e->info.gram_ms, &e->info.combine_ms, &e->info.residual_ms, &e->info.precond_ms};
        ++*cnt[ph];
        if (on) {
            IGX_HIP(hipEventRecord(e->ev[1], st));
            IGX_HIP(hipEventSynchronize(e->ev[1]));
            float t = 0.0f;
            (void)hipEventElapsedTime(&t, e->ev[0], e->ev[1]);
            *ms[ph] += t;
        }
        return IGX_OK;
    }
};

// yK = R K R^T x, yM = R M R^T x (x masked already); one of yK, yM may be null
int eig_products(hipStream_t st, igx_solver *s, EigState *e, int mb, const double *x, double *yK, double *yM)
{
    const int nm = (yK && yM) ? 2 : 1;
    int &nb = e->nb_spmm[eig_mb_slot(mb)][nm - 1];
    if (!nb) {
        int per_cu = 0;
        auto occupancy = [&](auto k) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, BLOCK, 0); };
        const hipError_t eo = s->mp ? with_csr_spmm2_kernel(s->gw, mb, nm, occupancy) : with_spmm2_kernel(s->gw, mb, nm, occupancy);
        if (eo != hipSuccess) { (void)hipGetLastError(); per_cu = 1; }
        nb = (int)std::min<long long>(NB_SPMV_MAX, (long long)std::max(1, per_cu) * std::max(1, s->ctx->ncu));
    }
    const long long groups = BLOCK / s->gw;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(nb, (s->n + groups - 1) / groups));
    if (const igx_multipatch *m = s->mp) {
        const double *vK = m->d_vals, *vM = s->d_mass;
        if (nm == 2) with_csr_spmm2_kernel(s->gw, mb, 2, [&](auto k) { k<<<grid, BLOCK, 0, st>>>(s->n, m->d_indptr, m->d_indices, vK, vM, s->d_mask, x, yK, yM); });
        else with_csr_spmm2_kernel(s->gw, mb, 1, [&](auto k) { k<<<grid, BLOCK, 0, st>>>(s->n, m->d_indptr, m->d_indices, yK ? vK : vM, nullptr, s->d_mask, x, yK ? yK : yM, nullptr); });
        IGX_HIP(hipGetLastError());
        return IGX_OK;
    }
    const double *vK = s->pv[IGX_ROLE_OPERATOR], *vM = s->pv[IGX_ROLE_MASS];
    if (nm == 2) with_spmm2_kernel(s->gw, mb, 2, [&](auto k) { k<<<grid, BLOCK, 0, st>>>(s->g, vK, vM, s->d_mask, x, yK, yM); });
    else with_spmm2_kernel(s->gw, mb, 1, [&](auto k) { k<<<grid, BLOCK, 0, st>>>(s->g, yK ? vK : vM, nullptr, s->d_mask, x, yK ? yK : yM, nullptr); });
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

// G (host, (na m) x (nb m)) = [A..]^T [B..] over the free rows
int eig_gram(hipStream_t st, igx_solver *s, EigState *e, int mb, int m, int na, const double *const *A, int nb, const double *const *B, double *G)
{
    GramArgs P{};
    for (int k = 0; k < 3; ++k) { P.A[k] = A[k < na ? k : 0]; P.B[k] = B[k < nb ? k : 0]; }
    P.na = na; P.nb = nb;
    const long long nchunk = (s->n + GR_RC - 1) / GR_RC;
    const int nblk = (int)std::max<long long>(1, std::min<long long>(NB_GRAM, nchunk));
    const int gw = 16 * ((3 * mb + 15) / 16);
    if (mb == 4) k_gram<4><<<nblk, BLOCK, 0, st>>>(s->n, P, s->d_mask, e->d_gpart);
    else if (mb == 8) k_gram<8><<<nblk, BLOCK, 0, st>>>(s->n, P, s->d_mask, e->d_gpart);
    else k_gram<16><<<nblk, BLOCK, 0, st>>>(s->n, P, s->d_mask, e->d_gpart);
    const int nout = na * m * nb * m;
    k_gram_fin<<<(nout + 255) / 256, 256, 0, st>>>(e->d_gpart, nblk, gw, mb, m, na, nb, e->d_small);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipMemcpyAsync(G, e->d_small, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

// the jobs of P with the m x m host coefficient blocks `coef` (ncoef of them, padded to mb x mb on the way up)
int eig_combine(hipStream_t st, igx_solver *s, EigState *e, int mb, int m, int njobs, const BlockComb &P, const double *coef, int ncoef)
{
    std::vector<double> h((size_t)ncoef * mb * mb, 0.0);
    for (int c = 0; c < ncoef; ++c)
        for (int a = 0; a < m; ++a)
            for (int b = 0; b < m; ++b) h[((size_t)c * mb + a) * mb + b] = coef[((size_t)c * m + a) * m + b];
    IGX_HIP(hipMemcpyAsync(e->d_small + EIG_COEF, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st));
    IGX_HIP(hipStreamSynchronize(st));                   // (h leaves scope)
    dim3 grid(vec_blocks(s->n), (unsigned)njobs);
    const double *dc = e->d_small + EIG_COEF;
    if (mb == 4) k_block_comb<4><<<grid, BLOCK, 0, st>>>(s->n, P, dc);
    else if (mb == 8) k_block_comb<8><<<grid, BLOCK, 0, st>>>(s->n, P, dc);
    else k_block_comb<16><<<grid, BLOCK, 0, st>>>(s->n, P, dc);
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

int eig_residuals(hipStream_t st, igx_solver *s, EigState *e, int mb, int m, const double *KX, const double *MX, const double *lam,
                  double *R, double *rnorm, double *knorm)
{
    double hl[EIG_MB_MAX] = {};
    std::copy(lam, lam + m, hl);
    IGX_HIP(hipMemcpyAsync(e->d_small + EIG_LAM, hl, sizeof(hl), hipMemcpyHostToDevice, st));
    IGX_HIP(hipStreamSynchronize(st));
    const unsigned nb = vec_blocks(s->n * mb);
    const double *dl = e->d_small + EIG_LAM;
    if (mb == 4) k_resid<4><<<nb, BLOCK, 0, st>>>(s->n, KX, MX, dl, s->d_mask, R, e->d_gpart);
    else if (mb == 8) k_resid<8><<<nb, BLOCK, 0, st>>>(s->n, KX, MX, dl, s->d_mask, R, e->d_gpart);
    else k_resid<16><<<nb, BLOCK, 0, st>>>(s->n, KX, MX, dl, s->d_mask, R, e->d_gpart);
    k_col_fin<<<1, 64, 0, st>>>(e->d_gpart, (int)nb, mb, e->d_small + EIG_NORM);
    IGX_HIP(hipGetLastError());
    double out[2 * EIG_MB_MAX] = {};
    IGX_HIP(hipMemcpyAsync(out, e->d_small + EIG_NORM, (size_t)2 * mb * sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < m; ++j) { rnorm[j] = std::sqrt(out[j]); knorm[j] = std::sqrt(out[mb + j]); }
    return IGX_OK;
}

// z = T r on blocks of mb columns: the fast-diagonalization inverse with batch = mb on the free box (z cleared outside it),
// Jacobi scaling, or the masked copy; a multipatch solver's V-cycle on the first m columns one after the other (the others: 0)
int eig_precond(hipStream_t st, igx_solver *s, EigState *e, int mb, int m, const double *r, double *z)
{
    const unsigned nb = vec_blocks(s->n * mb);
    if (e->precond == IGX_PRECOND_MG) {
        if (int rc = mg_check(s, "igx_solver_eig_precond")) return rc;
        if (m < mb) IGX_HIP(hipMemsetAsync(z, 0, (size_t)s->n * mb * sizeof(double), st));
        const unsigned nbv = vec_blocks(s->n);
        for (int j = 0; j < m; ++j) {
            k_block_col_get<<<nbv, BLOCK, 0, st>>>(s->n, mb, j, s->d_mask, r, s->w);
            IGX_HIP(hipGetLastError());
            if (int rc = mg_apply(st, s, s->w, s->z)) return rc;
            k_block_col_put<<<nbv, BLOCK, 0, st>>>(s->n, mb, j, s->z, z);
            IGX_HIP(hipGetLastError());
        }
        return IGX_OK;
    }
    if (e->precond == IGX_PRECOND_KRON) {
        const FastDiag F = box_fastdiag(s, 0, e->box_lo, e->box_nb, e->d_fac, e->lam_mode, mb);
        const long long wl = (long long)e->box_nb[0] * e->box_nb[1] * e->box_nb[2] * EIG_MB_MAX;
        double *W[2] = {e->d_W, e->d_W + wl};
        IGX_HIP(hipMemsetAsync(z, 0, (size_t)s->n * mb * sizeof(double), st));
        return apply_fastdiag(st, F, r, z, W);
    }
    k_block_scale<<<nb, BLOCK, 0, st>>>(s->n, mb, e->precond == IGX_PRECOND_JACOBI ? e->d_dinv : nullptr, s->d_mask, r, z);
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

bool eig_block_ok(int b) { return b >= 0 && b < EIG_NBLK; }

} // namespace

extern "C" {

int igx_solver_set_mass_d(igx_solver *s, double *d_M)
{
    const char *what = "igx_solver_set_mass_d";
    if (!s || !d_M) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->mp) { set_error("%s: needs a multipatch solver (a patch solver takes M with igx_solver_take_values)", what); return IGX_ERR_UNSUPPORTED; }
    if (d_M == s->mp->d_vals) { set_error("%s: the multipatch's own sums cannot be handed over (igx_multipatch_values_d copies them)", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    IGX_HIP(hipStreamSynchronize(s->ctx->stream));
    if (s->d_mass != d_M) (void)hipFree(s->d_mass);
    s->d_mass = d_M;
    return IGX_OK;
}

int igx_solver_eig_set_precond(igx_solver *s, int precond, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                               const double *const *lam, int lam_mode)
{
    const char *what = "igx_solver_eig_set_precond";
    EigState *e = nullptr;
    if (int rc = eig_state(s, what, &e)) return rc;
    hipStream_t st = s->ctx->stream;
    if (precond == IGX_PRECOND_NONE) { e->precond = precond; return IGX_OK; }
    if (precond == IGX_PRECOND_JACOBI) {
        if (!e->d_dinv) IGX_HIP(hipMalloc((void **)&e->d_dinv, (size_t)s->n * sizeof(double)));
        const unsigned nbd = (unsigned)((s->n + 255) / 256);
        if (s->mp) k_csr_diag<<<nbd, 256, 0, st>>>(s->n, s->mp->d_indptr, s->mp->d_indices, s->mp->d_vals, s->d_mask, e->d_dinv);
        else k_diag<<<nbd, 256, 0, st>>>(s->g, s->pv[IGX_ROLE_OPERATOR], s->d_mask, e->d_dinv);
        IGX_HIP(hipGetLastError());
        IGX_HIP(hipStreamSynchronize(st));
        e->precond = precond;
        return IGX_OK;
    }
    if (s->mp) {                              // a multipatch solver: the V-cycle of its hierarchy; no Kronecker, no Schwarz
        if (precond == IGX_PRECOND_KRON || precond == IGX_PRECOND_SCHWARZ) {
            set_error("%s: a multipatch solver's blocks take IGX_PRECOND_NONE, IGX_PRECOND_JACOBI or IGX_PRECOND_MG", what);
            return IGX_ERR_UNSUPPORTED;
        }
        if (precond != IGX_PRECOND_MG) { set_error("%s: unknown preconditioner %d", what, precond); return IGX_ERR_ARG; }
        if (int rc = mg_check(s, what)) return rc;
        e->precond = precond;
        return IGX_OK;
    }
    if (precond != IGX_PRECOND_KRON) { set_error("%s: unknown preconditioner %d", what, precond); return IGX_ERR_ARG; }
    int nb[3];
    if (int rc = box_fastdiag_setup(s, 0, box_lo, box_hi, U, lam, lam_mode, what, &e->precond, e->d_fac, nb)) return rc;
    (void)hipFree(e->d_W); e->d_W = nullptr;
    const size_t wl = (size_t)nb[0] * nb[1] * nb[2] * EIG_MB_MAX;
    IGX_HIP(hipMalloc((void **)&e->d_W, 2 * wl * sizeof(double)));
    for (int k = 0; k < 3; ++k) { e->box_lo[k] = k < s->dim ? box_lo[k] : 0; e->box_nb[k] = nb[k]; }
    e->lam_mode = lam_mode;
    e->precond = IGX_PRECOND_KRON;
    return IGX_OK;
}

int igx_solver_eig_begin(igx_solver *s, int m, const double *X0, int timed)
{
    const char *what = "igx_solver_eig_begin";
    EigState *e = nullptr;
    if (int rc = eig_state(s, what, &e)) return rc;
    if (!X0) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (m < 1 || m > EIG_MB_MAX) { set_error("%s: block of %d columns (1 to %d)", what, m, (int)EIG_MB_MAX); return IGX_ERR_ARG; }
    const int mb = m <= 4 ? 4 : m <= 8 ? 8 : 16;
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipStreamSynchronize(st));
    const size_t len = (size_t)s->n * mb, nblk = EIG_NBLK + EIG_NSCRATCH;
    if (e->mb != mb || !e->d_blocks) {
        (void)hipFree(e->d_blocks); e->d_blocks = nullptr;
        e->mb = e->m = 0;
        if (hipMalloc((void **)&e->d_blocks, nblk * len * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: out of device memory (%.3f GB)", what, nblk * len * 8.0 / 1e9);
            return IGX_ERR_NOMEM;
        }
    }
    for (size_t k = 0; k < nblk; ++k) e->blk[k] = e->d_blocks + k * len;
    IGX_HIP(hipMemsetAsync(e->d_blocks, 0, nblk * len * sizeof(double), st));
    // X0 padded to the row stride, its fixed rows cleared on the way
    std::vector<double> h(len, 0.0);
    for (long long I = 0; I < s->n; ++I)
        if (s->h_free[I])
            for (int j = 0; j < m; ++j) h[(size_t)I * mb + j] = X0[(size_t)I * m + j];
    IGX_HIP(hipMemcpyAsync(e->blk[IGX_EIG_X], h.data(), len * sizeof(double), hipMemcpyHostToDevice, st));
    IGX_HIP(hipStreamSynchronize(st));
    e->m = m; e->mb = mb; e->timed = timed != 0;
    e->info = igx_eig_info{};
    e->info.m = m; e->info.mb = mb;
    e->info.n_free = s->n - (long long)s->fixed.size();
    return IGX_OK;
}

int igx_solver_eig_products(igx_solver *s, int src, int dst_K, int dst_M)
{
    const char *what = "igx_solver_eig_products";
    EigState *e = nullptr;
    if (int rc = eig_session(s, what, &e)) return rc;
    if (!eig_block_ok(src) || (dst_K >= 0 && !eig_block_ok(dst_K)) || (dst_M >= 0 && !eig_block_ok(dst_M)) || (dst_K < 0 && dst_M < 0) ||
        src == dst_K || src == dst_M || dst_K == dst_M) {
        set_error("%s: bad blocks %d -> %d, %d", what, src, dst_K, dst_M);
        return IGX_ERR_ARG;
    }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_PRODUCTS, true);
    if (int rc = eig_products(st, s, e, e->mb, e->blk[src], dst_K >= 0 ? e->blk[dst_K] : nullptr, dst_M >= 0 ? e->blk[dst_M] : nullptr)) return rc;
    return ph.done();
}

int igx_solver_eig_gram(igx_solver *s, int na, const int32_t *a, int nb, const int32_t *b, double *G)
{
    const char *what = "igx_solver_eig_gram";
    EigState *e = nullptr;
    if (int rc = eig_session(s, what, &e)) return rc;
    if (!a || !b || !G || na < 1 || na > 3 || nb < 1 || nb > 3) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    const double *A[3] = {}, *B[3] = {};
    for (int k = 0; k < na; ++k) { if (!eig_block_ok(a[k])) { set_error("%s: bad block %d", what, a[k]); return IGX_ERR_ARG; } A[k] = e->blk[a[k]]; }
    for (int k = 0; k < nb; ++k) { if (!eig_block_ok(b[k])) { set_error("%s: bad block %d", what, b[k]); return IGX_ERR_ARG; } B[k] = e->blk[b[k]]; }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_GRAM, true);
    if (int rc = eig_gram(st, s, e, e->mb, e->m, na, A, nb, B, G)) return rc;
    return ph.done();
}

int igx_solver_eig_combine(igx_solver *s, int nupd, const int32_t *dst, const int32_t *nsrc, const int32_t *src, const double *coef,
                           int triple)
{
    const char *what = "igx_solver_eig_combine";
    EigState *e = nullptr;
    if (int rc = eig_session(s, what, &e)) return rc;
    if (!dst || !nsrc || !src || !coef || nupd < 1 || nupd > 2) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    const int per = triple ? 3 : 1;
    BlockComb P{};
    int njobs = 0, target[COMB_JOBS] = {};
    for (int u = 0; u < nupd; ++u) {
        const auto family = [&](int b) { return triple ? (b == IGX_EIG_X || b == IGX_EIG_W || b == IGX_EIG_P) : eig_block_ok(b); };
        if (nsrc[u] < 1 || nsrc[u] > 3 || !family(dst[u]) || (u == 1 && dst[1] == dst[0])) { set_error("%s: bad update %d", what, u); return IGX_ERR_ARG; }
        for (int j = 0; j < nsrc[u]; ++j)
            if (!family(src[3 * u + j])) { set_error("%s: bad source block %d", what, src[3 * u + j]); return IGX_ERR_ARG; }
        for (int c = 0; c < per; ++c, ++njobs) {
            for (int j = 0; j < nsrc[u]; ++j) P.S[njobs][j] = e->blk[src[3 * u + j] + c];
            P.Y[njobs] = e->blk[EIG_NBLK + njobs];
            P.nsrc[njobs] = nsrc[u];
            P.coef[njobs] = 3 * u;
            target[njobs] = dst[u] + c;
        }
    }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_COMBINE, true);
    // the coefficient blocks of update u at 3 u .. 3 u + nsrc[u] - 1 (slots past nsrc[u] are not read)
    std::vector<double> cf((size_t)3 * nupd * e->m * e->m, 0.0);
    const double *cp = coef;
    for (int u = 0; u < nupd; ++u)
        for (int j = 0; j < nsrc[u]; ++j, cp += (size_t)e->m * e->m) std::copy(cp, cp + (size_t)e->m * e->m, cf.begin() + (size_t)(3 * u + j) * e->m * e->m);
    if (int rc = eig_combine(st, s, e, e->mb, e->m, njobs, P, cf.data(), 3 * nupd)) return rc;
    for (int z = 0; z < njobs; ++z) std::swap(e->blk[target[z]], e->blk[EIG_NBLK + z]);
    return ph.done();
}

int igx_solver_eig_residuals(igx_solver *s, const double *lam, double *rnorm, double *knorm)
{
    const char *what = "igx_solver_eig_residuals";
    EigState *e = nullptr;
    if (int rc = eig_session(s, what, &e)) return rc;
    if (!lam || !rnorm || !knorm) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_RESID, true);
    if (int rc = eig_residuals(st, s, e, e->mb, e->m, e->blk[IGX_EIG_KX], e->blk[IGX_EIG_MX], lam, e->blk[IGX_EIG_R], rnorm, knorm)) return rc;
    return ph.done();
}

int igx_solver_eig_precond(igx_solver *s, int src, int dst)
{
    const char *what = "igx_solver_eig_precond";
    EigState *e = nullptr;
    if (int rc = eig_session(s, what, &e)) return rc;
    if (!eig_block_ok(src) || !eig_block_ok(dst) || src == dst) { set_error("%s: bad blocks %d -> %d", what, src, dst); return IGX_ERR_ARG; }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_PRECOND, true);
    if (int rc = eig_precond(st, s, e, e->mb, e->m, e->blk[src], e->blk[dst])) return rc;
    return ph.done();
}

int igx_solver_eig_download(igx_solver *s, int block, int k, double *out)
{
    const char *what = "igx_solver_eig_download";
    EigState *e = nullptr;
    if (int rc = eig_session(s, what, &e)) return rc;
    if (!out || !eig_block_ok(block) || k < 1 || k > e->m) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipMemcpy2DAsync(out, (size_t)k * sizeof(double), e->blk[block], (size_t)e->mb * sizeof(double), (size_t)k * sizeof(double),
                             (size_t)s->n, hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_solver_eig_info(igx_solver *s, igx_eig_info *info)
{
    const char *what = "igx_solver_eig_info";
    EigState *e = nullptr;
    if (int rc = eig_session(s, what, &e)) return rc;
    if (!info) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    *info = e->info;
    return IGX_OK;
}

int igx_solver_eig_end(igx_solver *s)
{
    const char *what = "igx_solver_eig_end";
    EigState *e = nullptr;
    if (int rc = eig_state(s, what, &e, false)) return rc;         // (a session ends over restarted sums as well)
    IGX_HIP(hipStreamSynchronize(s->ctx->stream));
    (void)hipFree(e->d_blocks); e->d_blocks = nullptr;
    e->m = e->mb = 0;
    return IGX_OK;
}

int igx_solver_eig_products_d(igx_solver *s, int mb, const double *d_X, double *d_YK, double *d_YM)
{
    const char *what = "igx_solver_eig_products_d";
    EigState *e = nullptr;
    if (int rc = eig_state(s, what, &e)) return rc;
    if (!eig_mb_ok(mb) || !d_X || (!d_YK && !d_YM) || !eig_aligned(d_X) || d_X == d_YK || d_X == d_YM || (d_YK && d_YK == d_YM)) {
        set_error("%s: bad argument (row stride 4, 8 or 16; 16-byte aligned, distinct buffers)", what);
        return IGX_ERR_ARG;
    }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_PRODUCTS, false);
    k_block_scale<<<vec_blocks(s->n * mb), BLOCK, 0, st>>>(s->n, mb, nullptr, s->d_mask, d_X, e->d_tmp);
    IGX_HIP(hipGetLastError());
    if (int rc = eig_products(st, s, e, mb, e->d_tmp, d_YK, d_YM)) return rc;
    IGX_HIP(hipStreamSynchronize(st));
    return ph.done();
}

int igx_solver_eig_gram_d(igx_solver *s, int mb, int m, int na, const double *const *d_A, int nb, const double *const *d_B, double *G)
{
    const char *what = "igx_solver_eig_gram_d";
    EigState *e = nullptr;
    if (int rc = eig_state(s, what, &e)) return rc;
    if (!eig_mb_ok(mb) || m < 1 || m > mb || !d_A || !d_B || !G || na < 1 || na > 3 || nb < 1 || nb > 3) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    for (int k = 0; k < na; ++k) if (!d_A[k]) { set_error("%s: null block", what); return IGX_ERR_ARG; }
    for (int k = 0; k < nb; ++k) if (!d_B[k]) { set_error("%s: null block", what); return IGX_ERR_ARG; }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_GRAM, false);
    if (int rc = eig_gram(st, s, e, mb, m, na, d_A, nb, d_B, G)) return rc;
    return ph.done();
}

int igx_solver_eig_combine_d(igx_solver *s, int mb, int m, int nsrc, const double *const *d_S, const double *coef, double *d_Y)
{
    const char *what = "igx_solver_eig_combine_d";
    EigState *e = nullptr;
    if (int rc = eig_state(s, what, &e)) return rc;
    if (!eig_mb_ok(mb) || m < 1 || m > mb || nsrc < 1 || nsrc > 3 || !d_S || !coef || !d_Y || !eig_aligned(d_Y)) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    BlockComb P{};
    for (int j = 0; j < nsrc; ++j) {
        if (!d_S[j] || d_S[j] == d_Y || !eig_aligned(d_S[j])) { set_error("%s: source %d is null, unaligned or the destination", what, j); return IGX_ERR_ARG; }
        P.S[0][j] = d_S[j];
    }
    P.Y[0] = d_Y; P.nsrc[0] = nsrc; P.coef[0] = 0;
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_COMBINE, false);
    if (int rc = eig_combine(st, s, e, mb, m, 1, P, coef, nsrc)) return rc;
    IGX_HIP(hipStreamSynchronize(st));
    return ph.done();
}

int igx_solver_eig_residuals_d(igx_solver *s, int mb, int m, const double *d_KX, const double *d_MX, const double *lam, double *d_R,
                               double *rnorm, double *knorm)
{
    const char *what = "igx_solver_eig_residuals_d";
    EigState *e = nullptr;
    if (int rc = eig_state(s, what, &e)) return rc;
    if (!eig_mb_ok(mb) || m < 1 || m > mb || !d_KX || !d_MX || !lam || !d_R || !rnorm || !knorm) { set_error("%s: bad argument", what); return IGX_ERR_ARG; }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_RESID, false);
    if (int rc = eig_residuals(st, s, e, mb, m, d_KX, d_MX, lam, d_R, rnorm, knorm)) return rc;
    return ph.done();
}

int igx_solver_eig_precond_d(igx_solver *s, int mb, const double *d_R, double *d_Z)
{
    const char *what = "igx_solver_eig_precond_d";
    EigState *e = nullptr;
    if (int rc = eig_state(s, what, &e)) return rc;
    if (!eig_mb_ok(mb) || !d_R || !d_Z || d_R == d_Z) { set_error("%s: bad argument (different buffers; row stride 4, 8 or 16)", what); return IGX_ERR_ARG; }
    hipStream_t st = s->ctx->stream;
    EigPhase ph(st, e, PH_PRECOND, false);
    if (int rc = eig_precond(st, s, e, mb, mb, d_R, d_Z)) return rc;              // (every column: a zero column comes out as zero)
    IGX_HIP(hipStreamSynchronize(st));
    return ph.done();
}

} // extern "C"
