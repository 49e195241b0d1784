// The block eigen-solver of generalized eigenproblems  K x = lam M x  on the device (igx_solver_eig_*, igx_solver_set_mass_d;
// DESIGN.md sections 22 and 23): the pieces of block LOBPCG on blocks of n rows and MB interleaved columns, driven by the host.
//   k_spmm2      the block product over the patch's structured layout: K and M times a block of interleaved columns in one pass
//                (DESIGN.md section 22).
//   k_csr_spmm2  the block product of the multipatch eigen-solver over the general CSR pattern: K and M times a block of
//                interleaved columns in one pass (k_spmm2 is its structured twin of section 22).
//   k_block_spmm2  the block product of a block solver's vector-valued form: the NC x NC blocks and one scalar M times a block of
//                interleaved columns of NC N rows in one launch.
//   k_gram, k_block_comb, k_resid, k_block_scale: Gram matrices, block combinations, residuals with their column norms and the
//                batched Jacobi scaling, all in a fixed summation order.
// Host side: one dispatch per block product (with_spmm2_kernel, with_csr_spmm2_kernel, with_block_spmm2_kernel) names the
// instantiations, for the launch and the occupancy query alike.  The solver structure, the row layout (Geom, row_hdr) and the fast-diagonalization and
// multigrid preconditioners come from solve.hip and multigrid.hip through solve_internal.h.
#include "solve_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace igx;

namespace igx {

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
    long long block_wl = 0;                   // a block solver: the length of one work buffer (its largest component box * EIG_MB_MAX)
    int nb_spmm[3][2] = {};                   // resident blocks of the block product per width and matrix count (0: not asked yet)
    hipEvent_t ev[2] = {};
    bool have_ev = false;
    igx_eig_info info{};
};

void eig_free(igx_solver *s)
{
    if (EigState *e = s->eig) {
        (void)hipFree(e->d_blocks); (void)hipFree(e->d_tmp); (void)hipFree(e->d_gpart); (void)hipFree(e->d_small);
        (void)hipFree(e->d_dinv); (void)hipFree(e->d_fac); (void)hipFree(e->d_W);
        if (e->have_ev)
            for (auto &ev : e->ev) (void)hipEventDestroy(ev);
        delete e;
    }
    (void)hipFree(s->d_mass);
}

void eig_drop_block_kron(igx_solver *s)
{
    if (s->eig && s->eig->precond == IGX_PRECOND_KRON) s->eig->precond = IGX_PRECOND_NONE;
}

} // namespace igx

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

// block (p, q) of the NC x NC blocks by a chain of uniform selects: p and q are loop variables, and an index into the by-value
// argument would put the pointers into scratch
template <int NC>
__device__ __forceinline__ const double *block_ptr(const BlockVals &A, int p, int q)
{
    const double *r = A.v[0];
#pragma unroll
    for (int k = 1; k < NC * NC; ++k) r = (p * NC + q == k) ? A.v[k] : r;
    return r;
}

// One walk of a lane through its entries of the row (k_spmm2's): acc[0 .. MB) += v0 . x, and (NW == 2) acc[MB .. 2 MB) += v1 . x,
// for the values v0 (and v1) of the row at `row` and the x-entries of the trial component that starts at xq.  A null v0 or v1
// (uniform over the grid) is not read and counts as zero: with NW == 2 the walks q != p add zeros to the sums of M.  That costs
// multiply-adds, of which the kernel has plenty to spare, and keeps one loop for every walk: with a loop of its own per case the
// sums did not stay in the same registers across them, and the kernel took 256 VGPRs at MB = 16.
template <int GW, int MB, int U, int NW>
__device__ __forceinline__ void block_row_walk(const double *__restrict__ v0, const double *__restrict__ v1, long long row, int len,
                                               const double *__restrict__ xq, int lane, int c, int bb, int a, int c1, int c2,
                                               int N12, int N2, double *acc)
{
    constexpr int H = MB / 2;
    const dbl2 zero2 = {0.0, 0.0};
    const int dc = GW % c2, db = (GW / c2) % c1, da = GW / (c1 * c2);
    for (int k0 = lane; k0 < len; k0 += U * GW) {
        double v[U][NW];
        dbl2 xv[U][H];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = k0 + u * GW < len;
            v[u][0] = (in && v0) ? __builtin_nontemporal_load(v0 + row + k0 + u * GW) : 0.0;
            if (NW == 2) v[u][NW - 1] = (in && v1) ? __builtin_nontemporal_load(v1 + row + k0 + u * GW) : 0.0;
            const dbl2 *xr = reinterpret_cast<const dbl2 *>(xq +(long long)(a * N12 + bb * N2 + c) * MB);
#pragma unroll
            for (int j = 0; j < H; ++j) xv[u][j] = in ? xr[j] : zero2;
            c += dc; bb += db; a += da;
            if (c >= c2) { c -= c2; ++bb; }
            if (bb >= c1) { bb -= c1; ++a; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int w = 0; w < NW; ++w)
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    acc[w * MB + 2 * j] += v[u][w] * xv[u][j].x;
                    acc[w * MB + 2 * j + 1] += v[u][w] * xv[u][j].y;
                }
    }
}

// The block product of a vector-valued form: blocks of NC N rows, component-major (entry (q N + J, j) at
// (q N + J) MB + j), and MB interleaved columns.
//   yK[(p N + I) MB + j] = free[p N + I] ? sum_q sum_J A_pq[I, J] x[(q N + J) MB + j] : 0
//   yM[(p N + I) MB + j] = free[p N + I] ?       sum_J M[I, J]   x[(p N + J) MB + j] : 0     (one scalar M for every component)
// NM == 2: both; NM == 1: K alone (vM null) or M alone (vM given; A is not read), written to yK.  One group of GW lanes serves a
// scalar row I (k_spmm2's row-to-group map, header one row ahead and lane walk) and keeps the NM MB sums of one test component p
// at a time: it walks the row once per trial component q whose block is present, and the M value joins the walk q == p, so every
// value of A_pq is read once (non-temporal), M at most NC times, and x_q comes from L2 again for every p.  Absent blocks (uniform
// over the grid) and the rows of fixed components (uniform over the group) are not read.  x must vanish on the fixed dofs.  The
// order of the sums is fixed (q ascending, then the walk, then ReduceScatter); no atomics.
template <int GW, int MB, int U, int NC, int NM>
__global__ void __launch_bounds__(BLOCK) k_block_spmm2(const Geom g, const BlockVals A, const double *__restrict__ vM,
                                                       const uint8_t *__restrict__ freem, const double *__restrict__ x,
                                                       double *__restrict__ yK, double *__restrict__ yM)
{
    constexpr int T = NM * MB;
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    const long long N = g.nrows;
    const int N1 = g.N[1], N2 = g.N[2];
    const int N12 = N1 * N2;
    const bool m_only = NM == 1 && vM != nullptr;
    long long I = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW;
    RowHdr h{};
    if (I < N) h = row_hdr(g, freem, I);
    for (; I < N; I += ngroups) {
        const RowHdr cur = h;
        if (I + ngroups < N) h = row_hdr(g, freem, I + ngroups);
        const int c0 = cur.c0 - cur.l0, c1 = cur.c1 - cur.l1, c2 = cur.c2 - cur.l2;
        const int len = c0 * c1 * c2;
        const long long row = igx_rowptr3(&cur.r0, &cur.r1, &cur.r2, g.S1, g.S2, c0, c1, 0, 0, 0);
        const long long xbase = (long long)(cur.l0 * N1 + cur.l1) * N2 + cur.l2;
        const int c = lane % c2, bb = (lane / c2) % c1, a = lane / (c1 * c2);
#pragma unroll 1
        for (int p = 0; p < NC; ++p) {
            const long long o = (p * N + I) * MB;
            if (!freem[p * N + I]) {                     // (uniform over the group)
                for (int j = lane; j < MB; j += GW) {
                    yK[o + j] = 0.0;
                    if (NM == 2) yM[o + j] = 0.0;
                }
                continue;
            }
            double acc[T];
#pragma unroll
            for (int i = 0; i < T; ++i) acc[i] = 0.0;
#pragma unroll 1
            for (int q = 0; q < NC; ++q) {
                const double *v0 = m_only ? (q == p ? vM : nullptr) : block_ptr<NC>(A, p, q);
                const double *v1 = (NM == 2 && q == p) ? vM : nullptr;
                if (!v0 && !v1) continue;                // (an absent block: uniform over the grid)
                block_row_walk<GW, MB, U, NM>(v0, v1, row, len, x + (q * N + xbase) * MB, lane, c, bb, a, c1, c2, N12, N2, acc);
            }
            int base = 0;
            ReduceScatter<GW, GW / 2, T>::run(acc, lane, base);
            constexpr int TF = T >= GW ? T / GW : 1;     // sums a writing lane holds: the original indices base .. base + TF - 1
            if (T >= GW || (lane & (GW / T - 1)) == 0) {
#pragma unroll
                for (int i = 0; i < TF; ++i) {
                    const int ob = base + i;             // (matrix, j) = (ob / MB, ob % MB); TF divides MB: one matrix per lane
                    double *y = (NM == 2 && ob >= MB) ? yM : yK;
                    y[o + (ob % MB)] = acc[i];
                }
            }
        }
    }
}

// f(the instantiation of the vector block product at group width gw) for a row stride MB, NM matrices and NC components: with
// with_block_spmm2_kernel the only place that names one (U as k_spmm2's)
template <int MB, int NM, int NC, class F>
decltype(auto) with_block_spmm2_gw(int gw, F &&f)
{
    switch (gw) {
    case 64: return f(k_block_spmm2<64, MB, 32 / MB, NC, NM>);
    case 32: return f(k_block_spmm2<32, MB, 16 / MB, NC, NM>);
    case 16: return f(k_block_spmm2<16, MB, 16 / MB, NC, NM>);
    case 8: return f(k_block_spmm2<8, MB, 16 / MB, NC, NM>);
    default: return f(k_block_spmm2<4, MB, 16 / MB, NC, NM>);
    }
}

template <int NM, int NC, class F>
decltype(auto) with_block_spmm2_mb(int gw, int mb, F &&f)
{
    switch (mb) {
    case 4: return with_block_spmm2_gw<4, NM, NC>(gw, f);
    case 8: return with_block_spmm2_gw<8, NM, NC>(gw, f);
    default: return with_block_spmm2_gw<16, NM, NC>(gw, f);
    }
}

template <class F>
decltype(auto) with_block_spmm2_kernel(int gw, int mb, int nm, int nc, F &&f)
{
    if (nc == 3) return nm == 2 ? with_block_spmm2_mb<2, 3>(gw, mb, f) : with_block_spmm2_mb<1, 3>(gw, mb, f);
    return nm == 2 ? with_block_spmm2_mb<2, 2>(gw, mb, f) : with_block_spmm2_mb<1, 2>(gw, mb, f);
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
    if (int rc = refuse_multipatch_block(s, what)) return rc;
    if (s->mp) {                              // K: the multipatch's current sums, M: the solver's own array
        if (!s->d_mass) { set_error("%s: a multipatch solver needs its mass matrix first (igx_solver_set_mass_d)", what); return IGX_ERR_ARG; }
        return values ? check_values(s, what) : IGX_OK;
    }
    if (s->ncomp > 1 && s->symmetric) {      // a block solver: K its blocks (every diagonal one present), M the mass it took
        if (int rc = check_values(s, what)) return rc;
        if (!s->block.mass) { set_error("%s: a block solver needs its mass matrix first (igx_solver_take_mass)", what); return IGX_ERR_ARG; }
        return IGX_OK;
    }
    if (!s->parabolic || !s->symmetric || s->ncomp != 1) {
        set_error("%s: needs a symmetric parabolic solver (igx_solver_create_parabolic) or a multipatch solver with a mass matrix "
                  "(igx_solver_set_mass_d)", what);
        return IGX_ERR_ARG;
    }
    if (!s->par.pv[IGX_ROLE_MASS] || !s->par.pv[IGX_ROLE_OPERATOR]) { set_error("%s: take M and K first (igx_solver_take_values)", what); return IGX_ERR_ARG; }
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
        const hipError_t eo = s->mp          ? with_csr_spmm2_kernel(s->gw, mb, nm, occupancy)
                              : s->ncomp > 1 ? with_block_spmm2_kernel(s->gw, mb, nm, s->ncomp, occupancy)
                                             : with_spmm2_kernel(s->gw, mb, nm, occupancy);
        if (eo != hipSuccess) { (void)hipGetLastError(); per_cu = 1; }
        nb = (int)std::min<long long>(NB_SPMV_MAX, (long long)std::max(1, per_cu) * std::max(1, s->ctx->ncu));
    }
    const long long groups = BLOCK / s->gw, rows = s->n / s->ncomp;      // (a block solver: one group per scalar row)
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(nb, (rows + groups - 1) / groups));
    if (s->ncomp > 1) {
        BlockVals A{};
        if (yK)
            for (int k = 0; k < s->ncomp * s->ncomp; ++k) A.v[k] = s->block.blk[k];
        const double *vM = yM ? s->block.mass : nullptr;
        with_block_spmm2_kernel(s->gw, mb, nm, s->ncomp, [&](auto k) { k<<<grid, BLOCK, 0, st>>>(s->g, A, vM, s->d_mask, x, yK ? yK : yM, nm == 2 ? yM : nullptr); });
        IGX_HIP(hipGetLastError());
        return IGX_OK;
    }
    if (const igx_multipatch *m = s->mp) {
        const double *vK = m->d_vals, *vM = s->d_mass;
        if (nm == 2) with_csr_spmm2_kernel(s->gw, mb, 2, [&](auto k) { k<<<grid, BLOCK, 0, st>>>(s->n, m->d_indptr, m->d_indices, vK, vM, s->d_mask, x, yK, yM); });
        else with_csr_spmm2_kernel(s->gw, mb, 1, [&](auto k) { k<<<grid, BLOCK, 0, st>>>(s->n, m->d_indptr, m->d_indices, yK ? vK : vM, nullptr, s->d_mask, x, yK ? yK : yM, nullptr); });
        IGX_HIP(hipGetLastError());
        return IGX_OK;
    }
    const double *vK = s->par.pv[IGX_ROLE_OPERATOR], *vM = s->par.pv[IGX_ROLE_MASS];
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
    if (e->precond == IGX_PRECOND_KRON && s->ncomp > 1) {        // diag(P_0, .., P_{nc-1}): each component's box, batch = mb
        double *W[2] = {e->d_W, e->d_W + e->block_wl};
        IGX_HIP(hipMemsetAsync(z, 0, (size_t)s->n * mb * sizeof(double), st));
        for (int c = 0; c < s->ncomp; ++c) {
            const BlockState &B = s->block;
            const FastDiag F = box_fastdiag(s, c * s->g.nrows, B.klo[c], B.knb[c], B.d_bkron[c], B.kmode[c], mb);
            if (int rc = apply_fastdiag(st, F, r, z, W)) return rc;
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
    if (int rc = refuse_multipatch_block(s, what)) return rc;
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
        if (s->ncomp > 1) {                   // component c: the diagonal of block (c, c) at offset c g.nrows
            for (int c = 0; c < s->ncomp; ++c) jacobi_diagonal(st, s, s->block.blk[c * s->ncomp + c], e->d_dinv + c * s->g.nrows, c);
        } else jacobi_diagonal(st, s, s->mp ? s->mp->d_vals : s->par.pv[IGX_ROLE_OPERATOR], e->d_dinv);
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
    if (s->ncomp > 1) {                       // a block solver: the factors of every component, set by igx_solver_set_block_kron
        if (box_lo || box_hi || U || lam) { set_error("%s: a block solver takes its Kronecker factors per component (igx_solver_set_block_kron): pass NULL here", what); return IGX_ERR_ARG; }
        long long nbox = 1;
        for (int c = 0; c < s->ncomp; ++c) {
            if (!s->block.d_bkron[c]) { set_error("%s: set the Kronecker factors of component %d first (igx_solver_set_block_kron)", what, c); return IGX_ERR_ARG; }
            nbox = std::max(nbox, (long long)s->block.knb[c][0] * s->block.knb[c][1] * s->block.knb[c][2]);
        }
        e->precond = IGX_PRECOND_NONE;
        IGX_HIP(hipStreamSynchronize(st));
        (void)hipFree(e->d_W); e->d_W = nullptr;
        e->block_wl = nbox * EIG_MB_MAX;
        IGX_HIP(hipMalloc((void **)&e->d_W, 2 * (size_t)e->block_wl * sizeof(double)));
        e->precond = IGX_PRECOND_KRON;
        return IGX_OK;
    }
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
