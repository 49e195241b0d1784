// Saddle-point systems  K = [[A, B^T], [B, 0]]  (Stokes) solved on the device with preconditioned MINRES (igx_solver_create_saddle,
// igx_solver_take_pair_block, igx_solver_set_saddle_schur, igx_solver_saddle_projection and the inspection calls
// igx_solver_download_pair_block, igx_solver_saddle_product_d, igx_solver_saddle_timing;
// include/igx.h).
//
// Replaces the host steps  scipy.sparse.bmat -> RestrictedLinearSystem -> spsolve  of the reference's solve-stokes notebook.  A is
// the nc x nc block matrix of a block solver over the velocity patch (solve.hip: its blocks, mask, vectors and Kronecker factors
// are reused), B = [B_0 .. B_{nc-1}] the rectangular matrices of a pair (pair.hip) whose rows are the pressure dofs.  Vectors have
// nc N_u + N_p entries, velocity components first.
//   k_pair_transpose  B_q^T in the pair layout of the swapped spaces (rows: velocity dofs, columns: the box of pressure dofs whose
//              support meets the row's), one thread per entry, an exact copy of the bits.  Made once per block: the transposed
//              product then streams its rows as the others do, without atomics and in a fixed order.
//   k_saddle_u velocity rows: y_p[I] = sum_q (A_pq x_q)[I] + (B_p^T x_pr)[I] -- k_block_spmv followed by the row of B_p^T, one group
//              of GW lanes per scalar row, one store of y.
//   k_saddle_p pressure rows: y_pr[i] = sum_q (B_q x_q)[i].
//              Both have the contract of k_spmv (b, sign, mask, optional dot partials) and their own dispatch tables.
//   MINRES     Paige and Saunders' recurrence as scipy.sparse.linalg.minres runs it, with one change of order: alfa = v.(A v) -
//              (beta / oldb) v.r1 from the partials of the product and of the update that formed v, instead of a pass of its own
//              over y - (beta / oldb) r1.  Lanczos, direction and iterate vectors stay in HBM; k_fin_minres forms alfa, beta, the
//              Givens rotation and phi on the device; the host reads the scalars back every check_every iterations.
#include "pair_internal.h"
#include "solve_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace igx;

namespace {

// the MINRES scalars (only k_fin_minres writes them).  MS_LAST: the update of this iteration is the final one (converged); the
// next k_fin_minres then sets MS_DONE, which freezes everything: iterations run past the stop (check_every > 1) change nothing.
enum { MS_BETA1 = 0, MS_BETA, MS_OLDB, MS_ALFA, MS_DBAR, MS_EPSLN, MS_OLDEPS, MS_DELTA, MS_CS, MS_SN, MS_PHI, MS_PHIBAR, MS_DENOM,
       MS_IT, MS_DONE, MS_LAST, MS_CONV, MS_REASON, MS_STOP, MS_SUM, MS_SUMSQ, MS_N = 24 };
enum { FM_INIT = 0, FM_ALFA, FM_BETA, FM_SUM };

struct RectVals {
    const double *v[3];
};

// B^T from B: thread (row J of B^T, offset o below the longest row of B^T) copies the entry (i, J) of B, which it finds from the
// tables of B as igx_rowptr3 does.  b: the layout of B (rows: N, columns: M), t: that of B^T (rows: M of b).  2D: a one-dof axis 0
template <int DIM>
__global__ void __launch_bounds__(256) k_pair_transpose(const RectGeom b, const RectGeom t, int maxrow, const double *__restrict__ B,
                                                        double *__restrict__ BT)
{
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long J = tid / maxrow;
    const int o = (int)(tid % maxrow);
    if (J >= t.nrows) return;
    int j[3];
    j[2] = (int)(J % t.N[2]);
    const long long r = J / t.N[2];
    j[1] = (int)(r % t.N[1]);
    j[0] = DIM == 3 ? (int)(r / t.N[1]) : 0;
    int lo[3], c[3];
    for (int k = 0; k < 3; ++k) { lo[k] = t.lo[k][j[k]]; c[k] = t.hi[k][j[k]] - lo[k]; }
    const int len = c[0] * c[1] * c[2];
    if (o >= len) return;
    int i[3], rem = o;
    i[2] = lo[2] + rem % c[2]; rem /= c[2];
    i[1] = lo[1] + rem % c[1]; rem /= c[1];
    i[0] = lo[0] + rem;
    const long long dst = igx_rowptr3(t.rp[0], t.rp[1], t.rp[2], t.S1, t.S2, c[0], c[1], j[0], j[1], j[2]) + o;
    int bl[3], bc[3];
    for (int k = 0; k < 3; ++k) { bl[k] = b.lo[k][i[k]]; bc[k] = b.hi[k][i[k]] - bl[k]; }
    const long long src = igx_rowptr3(b.rp[0], b.rp[1], b.rp[2], b.S1, b.S2, bc[0], bc[1], i[0], i[1], i[2]) +
                          ((long long)(j[0] - bl[0]) * bc[1] + (j[1] - bl[1])) * bc[2] + (j[2] - bl[2]);
    BT[dst] = B[src];
}

// what a row of a rectangular layout needs from its tables
struct RectRow {
    int c0, c1, c2, len, xbase;
    long long row;
};

__device__ __forceinline__ RectRow rect_row(const RectGeom &t, long long I)
{
    const int i2 = (int)(I % t.N[2]);
    const long long r = I / t.N[2];
    const int i1 = (int)(r % t.N[1]), i0 = (int)(r / t.N[1]);
    const int l0 = t.lo[0][i0], l1 = t.lo[1][i1], l2 = t.lo[2][i2];
    RectRow h;
    h.c0 = t.hi[0][i0] - l0; h.c1 = t.hi[1][i1] - l1; h.c2 = t.hi[2][i2] - l2;
    h.len = h.c0 * h.c1 * h.c2;
    h.row = igx_rowptr3(t.rp[0], t.rp[1], t.rp[2], t.S1, t.S2, h.c0, h.c1, i0, i1, i2);
    h.xbase = (l0 * t.M[1] + l1) * t.M[2] + l2;
    return h;
}

// Velocity rows of K x.  Vectors: x_q[J] = x[q N + J] (q < NC), x_pr[j] = x[NC N + j].  For the scalar row I, test component p:
// y[p N + I] = free[p N + I] ? (b ? b[p N + I] : 0) + s * (sum_q (A_pq x_q)[I] + (B_p^T x_pr)[I]) : 0, part[block] = sum of pd . y
// over the NC outputs of the rows of the block (optional).  The A part is k_block_spmv's loop (solve.hip); the row of B_p^T follows
// with the same lanes: x_pr gathered once for the NC outputs, the NC values of the entry streamed non-temporally.  Absent blocks
// (uniform over the grid) and the rows of fixed components (uniform over the group) are not read.
template <int GW, int U, int NC>
__global__ void __launch_bounds__(BLOCK) k_saddle_u(const Geom g, const BlockVals A, const RectGeom t, const RectVals BT,
                                                    const uint8_t *__restrict__ freem, const double *__restrict__ x, const double *b,
                                                    double s, double *y, const double *__restrict__ pd, double *part)
{
    __shared__ double sh[BLOCK];
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    const long long N = g.nrows;
    const int N1 = g.N[1], N2 = g.N[2];
    const int N12 = N1 * N2;
    const int M2 = t.M[2], M12 = t.M[1] * t.M[2];
    const double *__restrict__ xp = x + NC * N;
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
        double acc[NC];
#pragma unroll
        for (int p = 0; p < NC; ++p) acc[p] = 0.0;
        {
            const int c0 = cur.c0 - cur.l0, c1 = cur.c1 - cur.l1, c2 = cur.c2 - cur.l2;
            const int len = c0 * c1 * c2;
            const long long row = igx_rowptr3(&cur.r0, &cur.r1, &cur.r2, g.S1, g.S2, c0, c1, 0, 0, 0);
            const int xbase = (cur.l0 * N1 + cur.l1) * N2 + cur.l2;
            int c = lane % c2, bb = (lane / c2) % c1, a = lane / (c1 * c2);
            const int dc = GW % c2, db = (GW / c2) % c1, da = GW / (c1 * c2);
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
        }
        const RectRow tr = rect_row(t, I);
        if (tr.len > 0) {                            // (uniform over the group)
            const int c1 = tr.c1, c2 = tr.c2;
            int c = lane % c2, bb = (lane / c2) % c1, a = lane / (c1 * c2);
            const int dc = GW % c2, db = (GW / c2) % c1, da = GW / (c1 * c2);
            for (int k0 = lane; k0 < tr.len; k0 += U * GW) {
                double v[U][NC], xv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool in = k0 + u * GW < tr.len;
                    xv[u] = in ? xp[tr.xbase + a * M12 + bb * M2 + c] : 0.0;
#pragma unroll
                    for (int p = 0; p < NC; ++p)
                        v[u][p] = (in && fr[p]) ? __builtin_nontemporal_load(BT.v[p] + tr.row + k0 + u * GW) : 0.0;
                    c += dc; bb += db; a += da;
                    if (c >= c2) { c -= c2; ++bb; }
                    if (bb >= c1) { bb -= c1; ++a; }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int p = 0; p < NC; ++p) acc[p] += v[u][p] * xv[u];
            }
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

// Pressure rows of K x: y[i] = free[i] ? (b ? b[i] : 0) + s * sum_q (B_q x_q)[i] : 0 for the pressure dof i (freem, b, y and pd
// point at the pressure part of their vectors; x at the velocity part, x_q[J] = x[q N + J]), part[block] = sum of pd . y over the
// rows of the block (optional).  One group of GW lanes per row: x_q gathered once per entry for the NC blocks, whose values are
// streamed non-temporally.  Masked rows are not read.
template <int GW, int U, int NC>
__global__ void __launch_bounds__(BLOCK) k_saddle_p(const RectGeom g, const RectVals B, long long N, const uint8_t *__restrict__ freem,
                                                    const double *__restrict__ x, const double *b, double s, double *y,
                                                    const double *__restrict__ pd, double *part)
{
    __shared__ double sh[BLOCK];
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    const int M2 = g.M[2], M12 = g.M[1] * g.M[2];
    double dot = 0.0;
    for (long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW; I < g.nrows; I += ngroups) {
        if (!freem[I]) {                             // (uniform over the group)
            if (lane == 0) y[I] = 0.0;
            continue;
        }
        const RectRow tr = rect_row(g, I);
        double acc = 0.0;
        if (tr.len > 0) {
            const int c1 = tr.c1, c2 = tr.c2;
            int c = lane % c2, bb = (lane / c2) % c1, a = lane / (c1 * c2);
            const int dc = GW % c2, db = (GW / c2) % c1, da = GW / (c1 * c2);
            for (int k0 = lane; k0 < tr.len; k0 += U * GW) {
                double v[U][NC], xv[U][NC];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool in = k0 + u * GW < tr.len;
                    const long long J = tr.xbase + a * M12 + bb * M2 + c;
#pragma unroll
                    for (int q = 0; q < NC; ++q) {
                        xv[u][q] = in ? x[q * N + J] : 0.0;
                        v[u][q] = in ? __builtin_nontemporal_load(B.v[q] + tr.row + k0 + u * GW) : 0.0;
                    }
                    c += dc; bb += db; a += da;
                    if (c >= c2) { c -= c2; ++bb; }
                    if (bb >= c1) { bb -= c1; ++a; }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int q = 0; q < NC; ++q) acc += v[u][q] * xv[u][q];
            }
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

// f(the instantiation of a row kernel at group width gw for nc components): the only place that names one, for the launch and the
// occupancy query alike (U: NC^2 U values of the A part per lane in flight, as k_block_spmv)
template <class F>
decltype(auto) with_saddle_u_kernel(int gw, int nc, F &&f)
{
    if (nc == 3) {
        switch (gw) {
        case 64: return f(k_saddle_u<64, 2, 3>);
        case 32: return f(k_saddle_u<32, 2, 3>);
        case 16: return f(k_saddle_u<16, 2, 3>);
        case 8: return f(k_saddle_u<8, 2, 3>);
        default: return f(k_saddle_u<4, 2, 3>);
        }
    }
    switch (gw) {
    case 64: return f(k_saddle_u<64, 4, 2>);
    case 32: return f(k_saddle_u<32, 4, 2>);
    case 16: return f(k_saddle_u<16, 4, 2>);
    case 8: return f(k_saddle_u<8, 4, 2>);
    default: return f(k_saddle_u<4, 4, 2>);
    }
}

template <class F>
decltype(auto) with_saddle_p_kernel(int gw, int nc, F &&f)
{
    if (nc == 3) {
        switch (gw) {
        case 64: return f(k_saddle_p<64, 4, 3>);
        case 32: return f(k_saddle_p<32, 4, 3>);
        case 16: return f(k_saddle_p<16, 4, 3>);
        case 8: return f(k_saddle_p<8, 4, 3>);
        default: return f(k_saddle_p<4, 4, 3>);
        }
    }
    switch (gw) {
    case 64: return f(k_saddle_p<64, 4, 2>);
    case 32: return f(k_saddle_p<32, 4, 2>);
    case 16: return f(k_saddle_p<16, 4, 2>);
    case 8: return f(k_saddle_p<8, 4, 2>);
    default: return f(k_saddle_p<4, 4, 2>);
    }
}

// ---------------------------------------------------------------------------------------------
// vector kernels (grids of at most NB_VEC blocks, fixed trees: two solves give the same bits)

// y = d x
__global__ void k_mr_mul(long long n, const double *d, const double *x, double *y)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = d[i] * x[i];
}

// z = free ? scale z : 0 (the pressure part of the Kronecker preconditioner, masked again)
__global__ void k_mr_mask_scale(long long n, const uint8_t *freem, double scale, double *z)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) z[i] = freem[i] ? scale * z[i] : 0.0;
}

// y = a + b
__global__ void k_mr_add(long long n, const double *a, const double *b, double *y)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = a[i] + b[i];
}

// partA[block] = sum a b, partB[block] = sum a (b null: a a and a)
__global__ void __launch_bounds__(BLOCK) k_mr_dot(long long n, const double *a, const double *b, double *partA, double *partB)
{
    __shared__ double sh[BLOCK];
    double s1 = 0.0, s2 = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        s1 += a[i] * (b ? b[i] : a[i]);
        s2 += a[i];
    }
    s1 = block_sum(s1, sh);
    if (threadIdx.x == 0) partA[blockIdx.x] = s1;
    if (partB) {
        s2 = block_sum(s2, sh);
        if (threadIdx.x == 0) partB[blockIdx.x] = s2;
    }
}

// r -= free ? mean : 0 with mean = sc[MS_SUM] / n (the orthogonal projection off the constant pressure)
__global__ void k_mr_shift(long long n, const uint8_t *freem, const double *sc, double *r)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && freem[i]) r[i] -= sc[MS_SUM] / (double)n;
}

// v = y / beta (the first Lanczos vector)
__global__ void k_mr_first(long long n, const double *y, double *v, const double *sc)
{
    if (sc[MS_DONE] != 0.0) return;
    const double s = 1.0 / sc[MS_BETA];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) v[i] = s * y[i];
}

// r_new = y - (beta / oldb) r1 - (alfa / beta) r2, written over r1 (the host then exchanges r1 and r2)
__global__ void k_mr_lanczos(long long n, const double *y, double *r1, const double *r2, const double *sc)
{
    if (sc[MS_DONE] != 0.0 || sc[MS_LAST] != 0.0) return;
    const double c1 = sc[MS_IT] >= 1.0 ? sc[MS_BETA] / sc[MS_OLDB] : 0.0, c2 = sc[MS_ALFA] / sc[MS_BETA];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        r1[i] = (y[i] - c1 * r1[i]) - c2 * r2[i];
}

// w_new = (v - oldeps w1 - delta w2) denom, written over w1 (the host then exchanges w1 and w2); x += phi w_new; unless this update
// is the last one: v = y / beta, the next Lanczos vector, and the partials of v . r1 (r1: what the next iteration calls so)
__global__ void __launch_bounds__(BLOCK) k_mr_update(long long n, double *x, double *v, double *w1, const double *w2, const double *y,
                                                     const double *r1, const double *sc, double *part)
{
    __shared__ double sh[BLOCK];
    if (sc[MS_DONE] != 0.0) return;
    const double oldeps = sc[MS_OLDEPS], delta = sc[MS_DELTA], denom = sc[MS_DENOM], phi = sc[MS_PHI];
    const bool last = sc[MS_LAST] != 0.0;
    const double s = last ? 0.0 : 1.0 / sc[MS_BETA];
    double vr = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        const double wn = ((v[i] - oldeps * w1[i]) - delta * w2[i]) * denom;
        w1[i] = wn;
        x[i] += phi * wn;
        if (!last) {
            const double vn = s * y[i];
            v[i] = vn;
            vr += vn * r1[i];
        }
    }
    vr = block_sum(vr, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = vr;
}

// neither infinite nor NaN, from the exponent bits: a test by arithmetic (v - v == 0) does not survive the contraction of v's own
// product into an fma, which leaves the product's rounding error
__device__ __forceinline__ bool mr_finite(double v)
{
    return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

// one block: the sums of the partials in a fixed order, then the scalars of the step `op`
//   FM_SUM   sc[MS_SUM] = sum partA, sc[MS_SUMSQ] = sum partB
//   FM_INIT  partA: r1 . y -> beta1 = beta = phibar; everything else at its start value; stop = tol beta1
//   FM_ALFA  partA: v . (A v), partB: v . r1 -> alfa
//   FM_BETA  partA: r2 . y -> beta, the Givens rotation, phi, phibar; the stop and the breakdowns
__global__ void __launch_bounds__(BLOCK) k_fin_minres(const double *partA, int nA, const double *partB, int nB, double *sc, int op, double tol)
{
    __shared__ double sh[BLOCK];
    double a = 0.0, bsum = 0.0;
    for (int k = threadIdx.x; k < nA; k += BLOCK) a += partA[k];
    for (int k = threadIdx.x; k < nB; k += BLOCK) bsum += partB[k];
    a = block_sum(a, sh);
    bsum = block_sum(bsum, sh);
    if (threadIdx.x != 0) return;
    if (op == FM_SUM) { sc[MS_SUM] = a; sc[MS_SUMSQ] = bsum; return; }
    if (op == FM_INIT) {
        for (int k = 0; k < MS_SUM; ++k) sc[k] = 0.0;
        if (!mr_finite(a)) { sc[MS_DONE] = 1.0; sc[MS_REASON] = IGX_BREAKDOWN_NONFINITE; return; }
        if (a < 0.0) { sc[MS_DONE] = 1.0; sc[MS_REASON] = IGX_BREAKDOWN_INDEFINITE_PRECOND; return; }
        const double beta1 = sqrt(a);
        sc[MS_BETA1] = sc[MS_BETA] = sc[MS_PHIBAR] = beta1;
        sc[MS_CS] = -1.0;
        sc[MS_STOP] = tol * beta1;
        if (beta1 == 0.0) { sc[MS_DONE] = 1.0; sc[MS_CONV] = 1.0; }       // (the start vector solves the system)
        return;
    }
    if (sc[MS_DONE] != 0.0) return;
    if (sc[MS_LAST] != 0.0) { sc[MS_DONE] = 1.0; return; }
    if (op == FM_ALFA) {
        const double alfa = sc[MS_IT] >= 1.0 ? a - (sc[MS_BETA] / sc[MS_OLDB]) * bsum : a;
        if (!mr_finite(alfa)) { sc[MS_DONE] = 1.0; sc[MS_REASON] = IGX_BREAKDOWN_NONFINITE; return; }
        sc[MS_ALFA] = alfa;
        return;
    }
    // FM_BETA
    if (!mr_finite(a)) { sc[MS_DONE] = 1.0; sc[MS_REASON] = IGX_BREAKDOWN_NONFINITE; return; }
    if (a < 0.0) { sc[MS_DONE] = 1.0; sc[MS_REASON] = IGX_BREAKDOWN_INDEFINITE_PRECOND; return; }
    const double alfa = sc[MS_ALFA], oldb = sc[MS_BETA], beta = sqrt(a);
    const double cs = sc[MS_CS], sn = sc[MS_SN], dbar = sc[MS_DBAR];
    const double oldeps = sc[MS_EPSLN];
    const double delta = cs * dbar + sn * alfa;
    const double gbar = sn * dbar - cs * alfa;
    const double epsln = sn * beta;
    const double dbar_n = -cs * beta;
    double gamma = sqrt(gbar * gbar + beta * beta);
    gamma = fmax(gamma, 2.220446049250313e-16);
    const double cs_n = gbar / gamma, sn_n = beta / gamma;
    const double phi = cs_n * sc[MS_PHIBAR], phibar = sn_n * sc[MS_PHIBAR];
    if (!mr_finite(phi) || !mr_finite(phibar)) {
        sc[MS_DONE] = 1.0; sc[MS_REASON] = IGX_BREAKDOWN_NONFINITE; return;
    }
    sc[MS_OLDB] = oldb; sc[MS_BETA] = beta;
    sc[MS_OLDEPS] = oldeps; sc[MS_EPSLN] = epsln; sc[MS_DELTA] = delta; sc[MS_DBAR] = dbar_n;
    sc[MS_CS] = cs_n; sc[MS_SN] = sn_n;
    sc[MS_PHI] = phi; sc[MS_PHIBAR] = phibar;
    sc[MS_DENOM] = 1.0 / gamma;
    sc[MS_IT] += 1.0;
    if (fabs(phibar) <= sc[MS_STOP] || beta == 0.0) { sc[MS_LAST] = 1.0; sc[MS_CONV] = fabs(phibar) <= sc[MS_STOP] ? 1.0 : 0.0; }
}

unsigned blocks256(long long n) { return (unsigned)std::max<long long>(1, (n + 255) / 256); }

unsigned saddle_blocks(int nb_max, int gw, long long rows)
{
    const long long groups = BLOCK / gw;
    return (unsigned)std::max<long long>(1, std::min<long long>(nb_max, (rows + groups - 1) / groups));
}

BlockVals block_vals(const igx_solver *s)
{
    BlockVals A{};
    for (int k = 0; k < s->ncomp * s->ncomp; ++k) A.v[k] = s->block.hidden[k] ? nullptr : s->block.blk[k];
    return A;
}

// the rows [ilo, ihi) that hold column j, from the column ranges [jlo, jhi) of the rows: supports are monotone along an axis, so
// they are a range; false if the ranges given are not of that kind
bool transposed_ranges(const std::vector<int> &jlo, const std::vector<int> &jhi, int ncols, std::vector<int> &ilo, std::vector<int> &ihi,
                       std::vector<int> &rpt)
{
    const int nrows = (int)jlo.size();
    ilo.assign(ncols, nrows); ihi.assign(ncols, 0); rpt.assign(ncols + 1, 0);
    std::vector<int> count(ncols, 0);
    for (int i = 0; i < nrows; ++i) {
        if (jlo[i] < 0 || jhi[i] > ncols || jlo[i] > jhi[i]) return false;
        for (int j = jlo[i]; j < jhi[i]; ++j) { ilo[j] = std::min(ilo[j], i); ihi[j] = std::max(ihi[j], i + 1); ++count[j]; }
    }
    for (int j = 0; j < ncols; ++j) {
        if (count[j] == 0) ilo[j] = ihi[j] = 0;
        else if (ihi[j] - ilo[j] != count[j]) return false;
        rpt[j + 1] = rpt[j] + (ihi[j] - ilo[j]);
    }
    return true;
}

} // namespace

namespace igx {

int refuse_saddle(const igx_solver *s, const char *what)
{
    if (!s || !s->saddle) return IGX_OK;
    set_error("%s: a saddle-point solver (igx_solver_create_saddle) serves MINRES solves, the product and its block-diagonal "
              "preconditioner only", what);
    return IGX_ERR_UNSUPPORTED;
}

int saddle_check_values(const igx_solver *s, const char *what)
{
    for (int c = 0; c < s->ncomp; ++c) {
        if (!s->block.blk[c * s->ncomp + c]) {
            set_error("%s: diagonal block (%d, %d) of A missing: take it first (igx_solver_take_block)", what, c, c);
            return IGX_ERR_ARG;
        }
        if (!s->sad.B[c]) {
            set_error("%s: block B_%d missing: take it first (igx_solver_take_pair_block)", what, c);
            return IGX_ERR_ARG;
        }
    }
    return IGX_OK;
}

// y = free ? (b ? b : 0) + sign K x : 0 over all nc N_u + N_p rows: the velocity rows, then the pressure rows; the partials of pd . y
// of the first launch, then those of the second (saddle_partials of them in all)
int saddle_spmv(hipStream_t st, const igx_solver *s, const double *x, const double *b, double sign, double *y, const double *pd, double *part,
                hipEvent_t mid)
{
    const SaddleState &S = s->sad;
    const long long off = (long long)s->ncomp * S.nu;
    const unsigned nbu = saddle_blocks(S.nb_u, S.gw_u, S.nu), nbp = saddle_blocks(S.nb_p, S.gw_p, S.np);
    const BlockVals A = block_vals(s);
    RectVals B{}, BT{};
    for (int q = 0; q < s->ncomp; ++q) { B.v[q] = S.B[q]; BT.v[q] = S.BT[q]; }
    with_saddle_u_kernel(S.gw_u, s->ncomp, [&](auto k) { k<<<nbu, BLOCK, 0, st>>>(s->g, A, S.gT, BT, s->d_mask, x, b, sign, y, pd, part); });
    IGX_HIP(hipGetLastError());
    if (mid) IGX_HIP(hipEventRecord(mid, st));       // (between the two launches: igx_solver_saddle_product_d times them apart)
    with_saddle_p_kernel(S.gw_p, s->ncomp, [&](auto k) {
        k<<<nbp, BLOCK, 0, st>>>(S.gB, B, S.nu, s->d_mask + off, x, b ? b + off : nullptr, sign, y + off, pd ? pd + off : nullptr,
                                 part ? part + nbu : nullptr);
    });
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

static unsigned saddle_partials(const igx_solver *s)
{
    return saddle_blocks(s->sad.nb_u, s->sad.gw_u, s->sad.nu) + saddle_blocks(s->sad.nb_p, s->sad.gw_p, s->sad.np);
}

int saddle_set_precond(igx_solver *s, int precond)
{
    const char *what = "igx_solver_set_precond";
    if (precond == IGX_PRECOND_NONE) { s->precond = precond; return IGX_OK; }
    if (precond != IGX_PRECOND_JACOBI && precond != IGX_PRECOND_KRON) {
        set_error("%s: a saddle-point solver takes IGX_PRECOND_NONE, IGX_PRECOND_JACOBI or IGX_PRECOND_KRON, not %d", what, precond);
        return precond == IGX_PRECOND_SCHWARZ || precond == IGX_PRECOND_MG ? IGX_ERR_UNSUPPORTED : IGX_ERR_ARG;
    }
    if (s->sad.schur < 0) { set_error("%s: set the pressure part of the preconditioner first (igx_solver_set_saddle_schur)", what); return IGX_ERR_ARG; }
    if (precond == IGX_PRECOND_JACOBI) {
        if (int rc = saddle_check_values(s, what)) return rc;
        hipStream_t st = s->ctx->stream;
        for (int c = 0; c < s->ncomp; ++c) jacobi_diagonal(st, s, s->block.blk[c * s->ncomp + c], s->dinv + c * s->sad.nu, c);
        IGX_HIP(hipGetLastError());
        IGX_HIP(hipStreamSynchronize(st));
    } else {
        for (int c = 0; c < s->ncomp; ++c)
            if (!s->block.d_bkron[c]) {
                set_error("%s: set the Kronecker factors of component %d first (igx_solver_set_block_kron)", what, c);
                return IGX_ERR_ARG;
            }
    }
    s->precond = precond;
    return IGX_OK;
}

// z = diag(P_0, .., P_{nc-1}, P_S) r for r with zeros on the fixed dofs (z and r different vectors).  With the triangular variant
// selected (igx_solver_set_gmres; GMRES only): the solve with [[F, B^T], [0, -S]] -- z_p = -P_S r_p, then
// z_u = diag(P_0, ..) (r_u - B^T z_p), the B^T product by k_saddle_u with every block of A absent.
int saddle_apply_precond(hipStream_t st, igx_solver *s, const double *r, double *z)
{
    const SaddleState &S = s->sad;
    const long long nv = (long long)s->ncomp * S.nu;
    if (s->precond == IGX_PRECOND_NONE) {
        IGX_HIP(hipMemcpyAsync(z, r, (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, st));
        return IGX_OK;
    }
    double *W[2] = {s->d_W, s->d_W + s->wlen};
    const bool tri = s->gm.restart > 0 && s->gm.triangular;
    const double *ru = r;                            // what the velocity part is applied to
    if (tri) {
        double *t = S.d_mvec + 3 * s->n;
        if (S.schur == IGX_PRECOND_JACOBI) {
            k_mr_mul<<<blocks256(S.np), 256, 0, st>>>(S.np, S.d_sdinv, r + nv, z + nv);
            k_mr_mask_scale<<<blocks256(S.np), 256, 0, st>>>(S.np, s->d_mask + nv, -1.0, z + nv);
        } else {
            IGX_HIP(hipMemsetAsync(z + nv, 0, (size_t)S.np * sizeof(double), st));
            if (int rc = apply_fastdiag(st, S.skron, r, z, W)) return rc;
            k_mr_mask_scale<<<blocks256(S.np), 256, 0, st>>>(S.np, s->d_mask + nv, -S.sscale, z + nv);
        }
        // (the velocity part of z is read by the row kernel, against the zeros that stand for the absent blocks: it must be finite)
        IGX_HIP(hipMemsetAsync(z, 0, (size_t)nv * sizeof(double), st));
        RectVals BT{};
        for (int q = 0; q < s->ncomp; ++q) BT.v[q] = S.BT[q];
        const BlockVals none{};
        const unsigned nbu = saddle_blocks(S.nb_u, S.gw_u, S.nu);
        with_saddle_u_kernel(S.gw_u, s->ncomp, [&](auto k) {
            k<<<nbu, BLOCK, 0, st>>>(s->g, none, S.gT, BT, s->d_mask, z, r, -1.0, t, nullptr, nullptr);
        });
        IGX_HIP(hipGetLastError());
        ru = t;
    }
    if (s->precond == IGX_PRECOND_JACOBI) k_mr_mul<<<blocks256(nv), 256, 0, st>>>(nv, s->dinv, ru, z);
    else {
        if (!tri) IGX_HIP(hipMemsetAsync(z, 0, (size_t)nv * sizeof(double), st));
        for (int c = 0; c < s->ncomp; ++c)
            if (int rc = apply_fastdiag(st, s->block.bkron[c], ru, z, W)) return rc;
    }
    if (!tri) {
        if (S.schur == IGX_PRECOND_JACOBI) k_mr_mul<<<blocks256(S.np), 256, 0, st>>>(S.np, S.d_sdinv, r + nv, z + nv);
        else {
            IGX_HIP(hipMemsetAsync(z + nv, 0, (size_t)S.np * sizeof(double), st));
            if (int rc = apply_fastdiag(st, S.skron, r, z, W)) return rc;
            k_mr_mask_scale<<<blocks256(S.np), 256, 0, st>>>(S.np, s->d_mask + nv, S.sscale, z + nv);
        }
    }
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

void saddle_add(hipStream_t st, long long n, const double *a, const double *b, double *y)
{
    k_mr_add<<<blocks256(n), 256, 0, st>>>(n, a, b, y);
}

static int read_scalars(hipStream_t st, const igx_solver *s, double *h)
{
    IGX_HIP(hipMemcpyAsync(h, s->sad.d_msc, MS_N * sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

// the mean of the free pressure part of v is taken off it (s->sad.project); mean / norm out if not null
static int project_pressure(hipStream_t st, igx_solver *s, double *v, double *mean, double *norm)
{
    SaddleState &S = s->sad;
    const long long nv = (long long)s->ncomp * S.nu;
    const unsigned nbv = vec_blocks(S.np);
    double *pA = s->d_part, *pB = s->d_part + NB_SPMV_MAX;
    k_mr_dot<<<nbv, BLOCK, 0, st>>>(S.np, v + nv, nullptr, pB, pA);
    k_fin_minres<<<1, BLOCK, 0, st>>>(pA, (int)nbv, pB, (int)nbv, S.d_msc, FM_SUM, 0.0);
    if (S.project) k_mr_shift<<<blocks256(S.np), 256, 0, st>>>(S.np, s->d_mask + nv, S.d_msc, v + nv);
    IGX_HIP(hipGetLastError());
    if (mean || norm) {
        double h[MS_N];
        if (int rc = read_scalars(st, s, h)) return rc;
        if (mean) *mean = h[MS_SUM] / (double)S.np;
        if (norm) *norm = std::sqrt(h[MS_SUMSQ]);
    }
    return IGX_OK;
}

int saddle_project_vector(hipStream_t st, igx_solver *s, double *v) { return project_pressure(st, s, v, nullptr, nullptr); }

// ||v|| by the fixed-order two-pass sum
static int vector_norm(hipStream_t st, igx_solver *s, const double *v, double *norm)
{
    const unsigned nbv = vec_blocks(s->n);
    k_mr_dot<<<nbv, BLOCK, 0, st>>>(s->n, v, nullptr, s->d_part, nullptr);
    IGX_HIP(hipGetLastError());
    double rr = 0.0;
    if (int rc = sum_partials(st, s, nbv, &rr)) return rc;
    *norm = std::sqrt(rr);
    return IGX_OK;
}

// Preconditioned MINRES on R K R^T x = r0 (r0 in s->r, x the start vector).  Per iteration: y = K v (and v . K v), alfa,
// r_new = y - (beta / oldb) r1 - (alfa / beta) r2, y = P r_new (and r_new . y), beta and the rotation, w_new, x += phi w_new,
// v = y / beta (and v . r1).
static int solve_minres(hipStream_t st, igx_solver *s, double tol, int maxiter, int check_every, int timed, igx_solve_info &inf)
{
    SaddleState &S = s->sad;
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    const unsigned nbv = vec_blocks(n), nbs = saddle_partials(s);
    double *pS = s->d_part, *pV = s->d_part + NB_SPMV_MAX;        // (the products write at most NB_SPMV_MAX partials: see create)
    double *r1 = S.d_mvec, *r2 = r1 + n, *y = r2 + n, *v = y + n, *w1 = v + n, *w2 = w1 + n;
    IGX_HIP(hipMemcpyAsync(r1, s->r, nbytes, hipMemcpyDeviceToDevice, st));
    IGX_HIP(hipMemcpyAsync(r2, s->r, nbytes, hipMemcpyDeviceToDevice, st));
    IGX_HIP(hipMemsetAsync(w1, 0, 2 * nbytes, st));
    IGX_HIP(hipMemsetAsync(pV, 0, nbv * sizeof(double), st));       // (v . r1 of the first iteration: not formed, not used)
    if (int rc = saddle_apply_precond(st, s, r1, y)) return rc;
    k_mr_dot<<<nbv, BLOCK, 0, st>>>(n, r1, y, pS, nullptr);
    k_fin_minres<<<1, BLOCK, 0, st>>>(pS, (int)nbv, nullptr, 0, S.d_msc, FM_INIT, tol);
    k_mr_first<<<nbv, BLOCK, 0, st>>>(n, y, v, S.d_msc);
    IGX_HIP(hipGetLastError());
    double h[MS_N] = {};
    if (int rc = read_scalars(st, s, h)) return rc;
    hipEvent_t *E = s->ev;
    for (int it = 0; h[MS_DONE] == 0.0 && h[MS_LAST] == 0.0 && it < maxiter;) {
        ++it;
        if (timed) IGX_HIP(hipEventRecord(E[0], st));
        if (int rc = saddle_spmv(st, s, v, nullptr, 1.0, y, v, pS)) return rc;
        if (timed) IGX_HIP(hipEventRecord(E[1], st));
        k_fin_minres<<<1, BLOCK, 0, st>>>(pS, (int)nbs, pV, (int)nbv, S.d_msc, FM_ALFA, tol);
        k_mr_lanczos<<<nbv, BLOCK, 0, st>>>(n, y, r1, r2, S.d_msc);
        IGX_HIP(hipGetLastError());
        std::swap(r1, r2);                           // r2: the new Lanczos residual, r1: the one before
        if (timed) IGX_HIP(hipEventRecord(E[2], st));
        if (int rc = saddle_apply_precond(st, s, r2, y)) return rc;
        if (timed) IGX_HIP(hipEventRecord(E[3], st));
        k_mr_dot<<<nbv, BLOCK, 0, st>>>(n, r2, y, pS, nullptr);
        k_fin_minres<<<1, BLOCK, 0, st>>>(pS, (int)nbv, nullptr, 0, S.d_msc, FM_BETA, tol);
        k_mr_update<<<nbv, BLOCK, 0, st>>>(n, s->x, v, w1, w2, y, r1, S.d_msc, pV);
        IGX_HIP(hipGetLastError());
        std::swap(w1, w2);
        if (timed) IGX_HIP(hipEventRecord(E[4], st));
        if (timed || it % check_every == 0 || it == maxiter) {
            if (int rc = read_scalars(st, s, h)) return rc;
            if (timed) {
                float ms[4] = {};
                for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&ms[k], E[k], E[k + 1]);
                inf.spmv_ms += ms[0]; inf.precond_ms += ms[2]; inf.vector_ms += ms[1] + ms[3];
            }
        }
    }
    inf.iterations = (int)h[MS_IT];
    inf.converged = h[MS_CONV] != 0.0 ? 1 : 0;
    S.breakdown = (int)h[MS_REASON];
    return IGX_OK;
}

// The device entry of a saddle solve, as solve_lifted (solve.hip): b in s->b, `lift` = ext(g) (or null: nothing is lifted), the
// start vector in s->x if x0_in_x.  r = R (b - K lift), its pressure mean removed if the solver projects; MINRES; then the true
// relative residual from one more product.
int saddle_solve_lifted(hipStream_t st, igx_solver *s, const double *lift, bool x0_in_x, double tol, int maxiter, int check_every, int timed,
                        igx_solve_info &inf)
{
    SaddleState &S = s->sad;
    const long long n = s->n;
    if (s->method != IGX_METHOD_MINRES) { set_error("igx_solver_solve: a saddle-point solver solves with IGX_METHOD_MINRES"); return IGX_ERR_UNSUPPORTED; }
    if (!x0_in_x) IGX_HIP(hipMemsetAsync(s->x, 0, (size_t)n * sizeof(double), st));
    if (lift) {
        if (int rc = saddle_spmv(st, s, lift, s->b, -1.0, s->r, nullptr, nullptr)) return rc;
    } else mask_copy(st, s, s->b, s->r);
    if (int rc = project_pressure(st, s, s->r, &S.rhs_mean, &S.rhs_norm)) return rc;
    double bnorm = 0.0;
    if (int rc = vector_norm(st, s, s->r, &bnorm)) return rc;
    const double *rhs = s->r;                        // (GMRES forms the residual again at every restart: it keeps the right-hand side)
    if (x0_in_x) {
        if (s->gm.restart > 0) {
            IGX_HIP(hipMemcpyAsync(S.d_mvec, s->r, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
            rhs = S.d_mvec;
        }
        if (int rc = saddle_spmv(st, s, s->x, s->r, -1.0, s->r, nullptr, nullptr)) return rc;
    }
    if (s->gm.restart > 0) {
        if (int rc = solve_gmres(st, s, rhs, tol, maxiter, check_every, timed, inf)) return rc;
    } else if (int rc = solve_minres(st, s, tol, maxiter, check_every, timed, inf)) return rc;
    // the true residual R (b - K (ext(g) + x)), projected as the right-hand side was
    const double *full = s->x;
    if (lift) {
        k_mr_add<<<blocks256(n), 256, 0, st>>>(n, lift, s->x, s->p);
        IGX_HIP(hipGetLastError());
        full = s->p;
    }
    if (int rc = saddle_spmv(st, s, full, s->b, -1.0, s->q, nullptr, nullptr)) return rc;
    if (S.project)
        if (int rc = project_pressure(st, s, s->q, nullptr, nullptr)) return rc;
    double rnorm = 0.0;
    if (int rc = vector_norm(st, s, s->q, &rnorm)) return rc;
    inf.relres = bnorm > 0.0 ? rnorm / bnorm : 0.0;
    return IGX_OK;
}

} // namespace igx

// the tables lo | hi | rp of the three axes of a rectangular layout appended to tab (3D: a one-dof axis in front of a 2D one);
// their positions in pos[axis][0..2]
static void append_rect_tables(std::vector<int> &tab, int dim, const std::vector<int> *lo, const std::vector<int> *hi, const std::vector<int> *rp,
                               size_t pos[3][3])
{
    const int off = 3 - dim;
    for (int a = 0; a < 3; ++a) {
        const std::vector<int> one_lo{0}, one_hi{1}, one_rp{0, 1};
        const std::vector<int> &l = a < off ? one_lo : lo[a - off], &h = a < off ? one_hi : hi[a - off], &r = a < off ? one_rp : rp[a - off];
        pos[a][0] = tab.size(); tab.insert(tab.end(), l.begin(), l.end());
        pos[a][1] = tab.size(); tab.insert(tab.end(), h.begin(), h.end());
        pos[a][2] = tab.size(); tab.insert(tab.end(), r.begin(), r.end());
    }
}

static int saddle_occupancy(const igx_solver *s, bool pressure)
{
    int per_cu = 0;
    auto occupancy = [&](auto k) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, BLOCK, 0); };
    const hipError_t eo = pressure ? with_saddle_p_kernel(s->sad.gw_p, s->ncomp, occupancy) : with_saddle_u_kernel(s->sad.gw_u, s->ncomp, occupancy);
    if (eo != hipSuccess) { (void)hipGetLastError(); per_cu = 1; }
    // (half of NB_SPMV_MAX each: the partials of both launches of a product lie in one array of NB_SPMV_MAX)
    return (int)std::min<long long>(NB_SPMV_MAX / 2, (long long)std::max(1, per_cu) * std::max(1, s->ctx->ncu));
}

extern "C" {

int igx_solver_create_saddle(igx_patch *pt, igx_pair *pair, int ncomp, const int64_t *fixed, int64_t nfixed, igx_solver **out)
{
    const char *what = "igx_solver_create_saddle";
    if (!create_args_ok(pt, fixed, nfixed, out, what)) return IGX_ERR_ARG;
    if (!pair) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (ncomp != 2 && ncomp != 3) { set_error("%s: ncomp must be 2 or 3, not %d", what, ncomp); return IGX_ERR_ARG; }
    if (pair->pt != pt) { set_error("%s: the pair was made over another patch than patch_u", what); return IGX_ERR_ARG; }
    const int dim = pt->dim;
    // the transposed tables, on the host next to jlo / jhi / rp
    std::vector<int> ilo[3], ihi[3], rpt[3];
    long long maxB = 1, maxT = 1;
    for (int k = 0; k < dim; ++k) {
        if (!transposed_ranges(pair->jlo[k], pair->jhi[k], pt->ax[k].N, ilo[k], ihi[k], rpt[k])) {
            set_error("%s: axis %d: the column ranges of the pair are not monotone", what, k);
            return IGX_ERR_ARG;
        }
        int mb = 0, mt = 0;
        for (size_t i = 0; i < pair->jlo[k].size(); ++i) mb = std::max(mb, pair->jhi[k][i] - pair->jlo[k][i]);
        for (size_t j = 0; j < ilo[k].size(); ++j) mt = std::max(mt, ihi[k][j] - ilo[k][j]);
        maxB *= mb; maxT *= mt;
    }
    igx_solver *s = nullptr;
    if (int rc = create_patch_solver(pt, IGX_FORM, ncomp, false, fixed, nfixed, &s, what, pair->nrows)) return rc;
    s->saddle = true;
    s->symmetric = true;
    s->method = IGX_METHOD_MINRES;
    SaddleState &S = s->sad;
    S.pair = pair; S.nu = pt->nrows_total; S.np = pair->nrows; S.nnzB = pair->nnz;
    for (int k = 0; k < dim; ++k) S.Np[k] = pair->tax[k].N;
    // the longest row of each kernel: of A and of B^T for the velocity rows, of B for the pressure rows
    long long maxA = 1;
    for (int k = 0; k < dim; ++k) {
        int mc = 0;
        for (int i = 0; i < pt->ax[k].N; ++i) mc = std::max(mc, pt->ax[k].jhi[i] - pt->ax[k].jlo[i]);
        maxA *= mc;
    }
    S.maxT = maxT;
    S.gw_u = spmv_group_width(std::max(maxA, maxT));
    S.gw_p = spmv_group_width(maxB);
    S.nb_u = saddle_occupancy(s, false);
    S.nb_p = saddle_occupancy(s, true);
    std::vector<int> tab;
    size_t pb[3][3], ptt[3][3];
    append_rect_tables(tab, dim, pair->jlo, pair->jhi, pair->rp, pb);
    append_rect_tables(tab, dim, ilo, ihi, rpt, ptt);
    const size_t n = (size_t)s->n;
    bool ok = hipMalloc((void **)&S.d_rtab, tab.size() * sizeof(int)) == hipSuccess &&
              hipMalloc((void **)&S.d_mvec, 6 * n * sizeof(double)) == hipSuccess &&
              hipMalloc((void **)&S.d_msc, MS_N * sizeof(double)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); set_error("%s: out of device memory (%.3f GB)", what, 6.0 * 8 * n / 1e9); free_solver(s); return IGX_ERR_NOMEM;
    }
    hipStream_t st = s->ctx->stream;
    hipError_t e = hipMemcpyAsync(S.d_rtab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(S.d_mvec, 0, 6 * n * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(S.d_msc, 0, MS_N * sizeof(double), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); free_solver(s); return IGX_ERR_HIP; }
    const int off = 3 - dim;
    for (int a = 0; a < 3; ++a) {
        S.gB.N[a] = S.gT.M[a] = a < off ? 1 : pair->tax[a - off].N;
        S.gB.M[a] = S.gT.N[a] = a < off ? 1 : pt->ax[a - off].N;
        S.gB.lo[a] = S.d_rtab + pb[a][0]; S.gB.hi[a] = S.d_rtab + pb[a][1]; S.gB.rp[a] = S.d_rtab + pb[a][2];
        S.gT.lo[a] = S.d_rtab + ptt[a][0]; S.gT.hi[a] = S.d_rtab + ptt[a][1]; S.gT.rp[a] = S.d_rtab + ptt[a][2];
    }
    S.gB.S1 = tab[pb[1][2] + S.gB.N[1]]; S.gB.S2 = tab[pb[2][2] + S.gB.N[2]];
    S.gT.S1 = tab[ptt[1][2] + S.gT.N[1]]; S.gT.S2 = tab[ptt[2][2] + S.gT.N[2]];
    S.gB.nrows = S.np; S.gT.nrows = S.nu;
    *out = s;
    return IGX_OK;
}

int igx_solver_take_pair_block(igx_solver *s, igx_pair *pair, int q)
{
    const char *what = "igx_solver_take_pair_block";
    if (!s || !pair) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->saddle) { set_error("%s: not a saddle-point solver (igx_solver_create_saddle)", what); return IGX_ERR_ARG; }
    SaddleState &S = s->sad;
    if (pair != S.pair) { set_error("%s: not the pair the solver was made over", what); return IGX_ERR_ARG; }
    if (q < 0 || q >= s->ncomp) { set_error("%s: block %d of %d components", what, q, s->ncomp); return IGX_ERR_ARG; }
    if (S.B[q]) { set_error("%s: block %d was taken already", what, q); return IGX_ERR_ARG; }
    if (!pair->d_data) { set_error("%s: the pair holds no values: assemble them first (igx_pair_assemble, data_out may be NULL)", what); return IGX_ERR_ARG; }
    // thread (row of B^T, offset below its longest row)
    const long long maxT = std::max<long long>(1, S.maxT);
    const long long total = S.nu * maxT;
    if (total + 255 > 0xFFFFFFFFll) { set_error("%s: %lld threads in one launch exceed the grid limit", what, total); return IGX_ERR_UNSUPPORTED; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    IGX_HIP(hipStreamSynchronize(st));
    double *bt = nullptr;
    if (hipMalloc((void **)&bt, std::max<size_t>(1, (size_t)S.nnzB) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: hipMalloc of %.2f GB for the transposed values failed", what, S.nnzB * 8.0 / 1e9);
        return IGX_ERR_NOMEM;
    }
    // the transpose first: the values change hands only once B^T is whole, so that a failure leaves the pair as it was
    hipError_t e = hipEventRecord(s->ev[0], st);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((total + 255) / 256)), block(256);
        if (s->dim == 2) k_pair_transpose<2><<<grid, block, 0, st>>>(S.gB, S.gT, (int)maxT, pair->d_data, bt);
        else k_pair_transpose<3><<<grid, block, 0, st>>>(S.gB, S.gT, (int)maxT, pair->d_data, bt);
        e = hipGetLastError();
    }
    int rc = IGX_OK;
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); rc = IGX_ERR_HIP; }
    else rc = close_call(st, s->ev[0], s->ev[1], what, S.transpose_ms);
    if (rc) { (void)hipFree(bt); return rc; }
    S.B[q] = pair->d_data;                          // the buffer changes hands: the pair's next assembly allocates anew
    pair->d_data = nullptr;
    S.BT[q] = bt;
    return IGX_OK;
}

int igx_solver_saddle_product_d(igx_solver *s, const double *d_x, const double *d_b, double sign, const double *d_pd, double *d_y, double *dot)
{
    const char *what = "igx_solver_saddle_product_d";
    if (!s || !d_x || !d_y) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->saddle) { set_error("%s: not a saddle-point solver (igx_solver_create_saddle)", what); return IGX_ERR_ARG; }
    if (d_x == d_y) { set_error("%s: d_x and d_y must be different buffers", what); return IGX_ERR_ARG; }
    if (int rc = saddle_check_values(s, what)) return rc;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    SaddleState &S = s->sad;
    IGX_HIP(hipEventRecord(s->ev[0], st));
    if (int rc = saddle_spmv(st, s, d_x, d_b, sign, d_y, d_pd, d_pd ? s->d_part : nullptr, s->ev[1])) return rc;
    float total = 0.0f;
    if (int rc = close_call(st, s->ev[0], s->ev[2], what, total)) return rc;
    (void)hipEventElapsedTime(&S.u_ms, s->ev[0], s->ev[1]);
    (void)hipEventElapsedTime(&S.p_ms, s->ev[1], s->ev[2]);
    if (dot) {
        *dot = 0.0;
        if (d_pd)
            if (int rc = sum_partials(st, s, saddle_partials(s), dot)) return rc;
    }
    return IGX_OK;
}

// --- the correction form of a nonlinear saddle-point iteration: the iterate is the caller's device vector,
// the residual stays in s->b between the two calls, so that the blocks may be replaced in between (Newton: the residual is that
// of the Picard matrix, the correction is solved with the Newton matrix)
static int saddle_gmres_ok(const igx_solver *s, const char *what)
{
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->saddle) { set_error("%s: not a saddle-point solver (igx_solver_create_saddle)", what); return IGX_ERR_ARG; }
    if (s->gm.restart <= 0) { set_error("%s: the solver does not run GMRES (igx_solver_set_gmres)", what); return IGX_ERR_UNSUPPORTED; }
    return saddle_check_values(s, what);
}

int igx_solver_saddle_residual_d(igx_solver *s, const double *d_b, const double *d_x, double *norm)
{
    const char *what = "igx_solver_saddle_residual_d";
    if (int rc = saddle_gmres_ok(s, what)) return rc;
    if (!d_x || !norm) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (d_x == s->b || d_b == s->b) { set_error("%s: d_x and d_b must not be the solver's own vectors", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    // r = R (b - K x) by the row kernels, x unmasked (it carries the Dirichlet values); projected as a solve projects its right-hand side
    if (int rc = saddle_spmv(st, s, d_x, d_b, -1.0, s->b, nullptr, nullptr)) return rc;
    if (s->sad.project)
        if (int rc = project_pressure(st, s, s->b, nullptr, nullptr)) return rc;
    return vector_norm(st, s, s->b, norm);
}

int igx_solver_saddle_correct_d(igx_solver *s, double *d_x, double tol, int maxiter, int check_every, int timed, igx_solve_info *info)
{
    const char *what = "igx_solver_saddle_correct_d";
    if (int rc = saddle_gmres_ok(s, what)) return rc;
    if (!d_x) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!(tol >= 0.0) || maxiter < 0) { set_error("%s: tol must be >= 0 and maxiter >= 0", what); return IGX_ERR_ARG; }
    if (check_every < 1) check_every = 1;
    s->sad.breakdown = 0;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    igx_solve_info inf{};
    IGX_HIP(hipEventRecord(s->ev[5], st));
    // nothing is lifted: the correction vanishes on the fixed dofs, the right-hand side is the residual in s->b, GMRES starts from zero
    // A projecting solver: the constant pressure is the kernel of the continuous operator, but on a NURBS geometry only nearly that
    // of the discrete one (B^T 1 is the quadrature error of int div v, 1e-9 on the golden case).  Left alone, GMRES resolves that
    // direction once the residual is small enough: corrections with pressures of 1e3 and a velocity 1e-4 off.  The correction
    // therefore runs on Q K Q and Q P, Q taking the pressure mean off: exactly singular, consistent, its solution mean-free.
    s->gm.project_ops = s->sad.project ? 1 : 0;
    const int rc_solve = saddle_solve_lifted(st, s, nullptr, false, tol, maxiter, check_every, timed, inf);
    s->gm.project_ops = 0;
    if (rc_solve) return rc_solve;
    k_mr_add<<<blocks256(s->n), 256, 0, st>>>(s->n, d_x, s->x, d_x);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipEventRecord(s->ev[4], st));
    IGX_HIP(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&inf.total_ms, s->ev[5], s->ev[4]);
    inf.n_free = s->n - (long long)s->fixed.size();
    if (info) *info = inf;
    return IGX_OK;
}

int igx_solver_saddle_timing(const igx_solver *s, float *transpose_ms, float *u_rows_ms, float *p_rows_ms)
{
    if (!s || !s->saddle) { set_error("igx_solver_saddle_timing: not a saddle-point solver (igx_solver_create_saddle)"); return IGX_ERR_ARG; }
    if (transpose_ms) *transpose_ms = s->sad.transpose_ms;
    if (u_rows_ms) *u_rows_ms = s->sad.u_ms;
    if (p_rows_ms) *p_rows_ms = s->sad.p_ms;
    return IGX_OK;
}

int igx_solver_download_pair_block(const igx_solver *s, int q, int transposed, double *vals)
{
    const char *what = "igx_solver_download_pair_block";
    if (!s || !vals) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->saddle) { set_error("%s: not a saddle-point solver (igx_solver_create_saddle)", what); return IGX_ERR_ARG; }
    if (q < 0 || q >= s->ncomp || !s->sad.B[q]) { set_error("%s: block %d is absent", what, q); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    IGX_HIP(hipMemcpyAsync(vals, transposed ? s->sad.BT[q] : s->sad.B[q], (size_t)s->sad.nnzB * sizeof(double), hipMemcpyDeviceToHost, s->ctx->stream));
    IGX_HIP(hipStreamSynchronize(s->ctx->stream));
    return IGX_OK;
}

int igx_solver_set_saddle_schur(igx_solver *s, int mode, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                                const double *const *lam, int lam_mode, const double *dinv, double scale)
{
    const char *what = "igx_solver_set_saddle_schur";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->saddle) { set_error("%s: not a saddle-point solver (igx_solver_create_saddle)", what); return IGX_ERR_ARG; }
    if (!(scale > 0.0) || scale - scale != 0.0) { set_error("%s: scale must be positive and finite", what); return IGX_ERR_ARG; }
    SaddleState &S = s->sad;
    const long long nv = (long long)s->ncomp * S.nu;
    if (mode != IGX_PRECOND_KRON && mode != IGX_PRECOND_JACOBI) {
        set_error("%s: mode must be IGX_PRECOND_KRON or IGX_PRECOND_JACOBI, not %d", what, mode);
        return IGX_ERR_ARG;
    }
    if (mode == IGX_PRECOND_JACOBI && !dinv) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    // the pressure part in use is replaced: no preconditioner is selected until igx_solver_set_precond selects one again,
    // whatever fails below
    S.schur = -1;
    s->precond = IGX_PRECOND_NONE;
    if (mode == IGX_PRECOND_JACOBI) {
        std::vector<double> h((size_t)S.np);
        for (long long i = 0; i < S.np; ++i) h[i] = s->h_free[nv + i] ? scale * dinv[i] : 0.0;
        IGX_HIP(hipStreamSynchronize(st));
        if (int rc = upload_replacing(st, h, S.d_sdinv)) return rc;
        IGX_HIP(hipStreamSynchronize(st));
        S.schur = mode; S.sscale = scale;
        return IGX_OK;
    }
    int nb[3];
    if (int rc = box_fastdiag_setup(s, nv, box_lo, box_hi, U, lam, lam_mode, what, nullptr, S.d_skron, nb, S.Np, false)) return rc;
    const long long nbox = (long long)nb[0] * nb[1] * nb[2];
    if (nbox > s->wlen)
        if (int rc = alloc_fastdiag_work(s, nbox)) return rc;
    S.skron = box_fastdiag(s, nv, box_lo, nb, S.d_skron, lam_mode, 1, S.Np);
    S.swlen = nbox;
    S.schur = mode; S.sscale = scale;
    return IGX_OK;
}

int igx_solver_saddle_projection(igx_solver *s, int enable, double *mean, double *norm)
{
    const char *what = "igx_solver_saddle_projection";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->saddle) { set_error("%s: not a saddle-point solver (igx_solver_create_saddle)", what); return IGX_ERR_ARG; }
    if (enable > 0) {
        const long long nv = (long long)s->ncomp * s->sad.nu;
        for (long long i = 0; i < s->sad.np; ++i)
            if (!s->h_free[nv + i]) {
                set_error("%s: pressure dof %lld is fixed: the constant pressure is not in the kernel, nothing to project", what, i);
                return IGX_ERR_ARG;
            }
    }
    if (enable >= 0) s->sad.project = enable > 0;
    if (mean) *mean = s->sad.rhs_mean;
    if (norm) *norm = s->sad.rhs_norm;
    return IGX_OK;
}

} // extern "C"
