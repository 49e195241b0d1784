// The smoother of the geometric multigrid for multipatch block solvers (igx_solver_set_block_mg_*): a
// coloured node-block Gauss-Seidel sweep over the NC x NC blocks A_pq of a vector-valued form, which share the global CSR pattern
// of the multipatch.  A node is a scalar global dof I with its NC components x_p[I] = x[p N + I].
//   k_csr_node_gs   one colour of a sweep: the row loop of k_csr_block_spmv (one group of GW lanes per node, the column index
//                   loaded once per entry, the values of the present blocks streamed once, x_q[J] gathered for every trial
//                   component) over the nodes of the colour.  The lane that meets J == I keeps its NC x NC values as the diagonal
//                   block D instead of adding them; the group leader solves D_FF x_F[I] = b_F[I] - sum_{J != I} sum_q
//                   A_Fq[I,J] x_q[J] - sum_{q fixed} D_Fq x_q[I] on the free components F of the node and writes them.  Nodes of
//                   one colour never couple, so one launch per colour in stream order is the sequential block sweep in
//                   (colour, index) order.
// The levels, the transfers and the cycle are those of multigrid.hip, which launches the sweep through csr_node_gs_sweep.
#include "mg_internal.h"

#include <algorithm>

using namespace igx;

namespace {

constexpr int BLOCK = 256;
// blocks of one colour's launch (grid-stride over the nodes of the colour): 2048 blocks of 4 waves are the 32 wave slots of each
// of the 256 compute units (the kernel's registers admit 5 waves per SIMD, 1280 blocks), so a larger grid adds no resident waves
constexpr int NB_NODE_GS_MAX = 2048;

struct NodeBlocks {
    const double *v[9];                       // block (p, q) at p * NC + q over the CSR pattern, or null (absent: zero)
};

// The nodes rows[0 .. nr) of one colour.  freem: the mask over the NC * N blocked dofs; sym: the form is symmetric, and D_qp is
// taken from D_pq (p < q; the diagonal entry of A_qp equals that of A_pq), which makes D symmetric bit for bit.
template <int GW, int U, int NC>
__global__ void __launch_bounds__(BLOCK) k_csr_node_gs(long long nr, const int32_t *__restrict__ rows, long long N,
                                                       const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                       const NodeBlocks A, const uint8_t *__restrict__ freem, double *x,
                                                       const double *__restrict__ b, int sym)
{
    const int lane = threadIdx.x % GW;
    const long long ngroups = (long long)gridDim.x * (BLOCK / GW);
    for (long long r = (long long)blockIdx.x * (BLOCK / GW) + threadIdx.x / GW; r < nr; r += ngroups) {
        const long long I = rows[r];
        int fr = 0;
#pragma unroll
        for (int p = 0; p < NC; ++p) fr |= (freem[p * N + I] != 0) << p;
        if (!fr) continue;                           // (uniform over the group; the colour lists hold no such node)
        const long long k0 = indptr[I], k1 = indptr[I + 1];
        double acc[NC], D[NC][NC];
#pragma unroll
        for (int p = 0; p < NC; ++p) {
            acc[p] = 0.0;
#pragma unroll
            for (int q = 0; q < NC; ++q) D[p][q] = 0.0;
        }
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
                        const double *vp = A.v[p * NC + q];          // (null or not: uniform over the grid)
                        v[u][p][q] = (in && ((fr >> p) & 1) && vp) ? __builtin_nontemporal_load(vp + k + u * GW) : 0.0;
                    }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < NC; ++q) xv[u][q] = (c[u] >= 0 && c[u] != I) ? x[q * N + c[u]] : 0.0;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int p = 0; p < NC; ++p)
#pragma unroll
                    for (int q = 0; q < NC; ++q) {
                        acc[p] += v[u][p][q] * xv[u][q];
                        if (c[u] == I) D[p][q] += v[u][p][q];
                    }
        }
        // (one lane of the group met J == I: every other lane adds zeros to D, so its sum is exact)
#pragma unroll
        for (int off = GW / 2; off > 0; off >>= 1)
#pragma unroll
            for (int p = 0; p < NC; ++p) {
                acc[p] += __shfl_xor(acc[p], off, GW);
#pragma unroll
                for (int q = 0; q < NC; ++q) D[p][q] += __shfl_xor(D[p][q], off, GW);
            }
        if (lane != 0) continue;
        if (sym) {
#pragma unroll
            for (int p = 0; p < NC; ++p)
#pragma unroll
                for (int q = p + 1; q < NC; ++q)
                    if ((fr >> p) & 1) D[q][p] = D[p][q];            // (row p was read; a fixed row p was not)
        }
        double rhs[NC];
#pragma unroll
        for (int p = 0; p < NC; ++p) rhs[p] = ((fr >> p) & 1) ? b[p * N + I] - acc[p] : 0.0;
        // a fixed component q keeps its entry: its column goes to the right-hand side, its row and column become the identity's
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            if ((fr >> q) & 1) continue;
            const double xq = x[q * N + I];
#pragma unroll
            for (int p = 0; p < NC; ++p) {
                if ((fr >> p) & 1) rhs[p] -= D[p][q] * xq;
                D[p][q] = 0.0;
                D[q][p] = 0.0;
            }
            D[q][q] = 1.0;
        }
        // elimination in the order of the components, without pivoting (D_FF of a positive definite form is positive definite)
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const double piv = D[k][k];
            ok = ok && piv != 0.0 && __builtin_isfinite(piv);
#pragma unroll
            for (int i = k + 1; i < NC; ++i) {
                const double f = D[i][k] / piv;
#pragma unroll
                for (int j = k + 1; j < NC; ++j) D[i][j] -= f * D[k][j];
                rhs[i] -= f * rhs[k];
            }
        }
        if (!ok) continue;                           // (a zero or non-finite pivot leaves the node as it is)
        double y[NC];
#pragma unroll
        for (int k = NC - 1; k >= 0; --k) {
            double t = rhs[k];
#pragma unroll
            for (int j = k + 1; j < NC; ++j) t -= D[k][j] * y[j];
            y[k] = t / D[k][k];
        }
#pragma unroll
        for (int p = 0; p < NC; ++p)
            if ((fr >> p) & 1) x[p * N + I] = y[p];
    }
}

// f(the sweep kernel at group width gw and nc components): the widths and batches of k_csr_block_spmv
template <class F>
decltype(auto) with_csr_node_gs_kernel(int gw, int nc, F &&f)
{
    if (nc == 3) {
        switch (gw) {
        case 64: return f(k_csr_node_gs<64, 2, 3>);
        case 32: return f(k_csr_node_gs<32, 2, 3>);
        case 16: return f(k_csr_node_gs<16, 2, 3>);
        case 8: return f(k_csr_node_gs<8, 2, 3>);
        default: return f(k_csr_node_gs<4, 2, 3>);
        }
    }
    switch (gw) {
    case 64: return f(k_csr_node_gs<64, 4, 2>);
    case 32: return f(k_csr_node_gs<32, 4, 2>);
    case 16: return f(k_csr_node_gs<16, 4, 2>);
    case 8: return f(k_csr_node_gs<8, 4, 2>);
    default: return f(k_csr_node_gs<4, 4, 2>);
    }
}

} // namespace

namespace igx {

int csr_node_gs_sweep(hipStream_t st, int gw, int nc, int ncol, const int *coff, const int32_t *d_rows, long long N,
                      const int32_t *d_indptr, const int32_t *d_indices, const double *const *blk, const uint8_t *d_mask, bool sym,
                      double *x, const double *b, bool backward, int *launches)
{
    if (nc != 2 && nc != 3) { set_error("csr_node_gs_sweep: %d components (2 or 3)", nc); return IGX_ERR_ARG; }
    NodeBlocks A{};
    for (int k = 0; k < nc * nc; ++k) A.v[k] = blk[k];
    const long long groups = BLOCK / gw;
    for (int ci = 0; ci < ncol; ++ci) {
        const int c = backward ? ncol - 1 - ci : ci;
        const long long nr = coff[c + 1] - coff[c];
        if (nr == 0) continue;
        const unsigned nb = (unsigned)std::min<long long>(NB_NODE_GS_MAX, (nr + groups - 1) / groups);
        with_csr_node_gs_kernel(gw, nc, [&](auto k) {
            k<<<nb, BLOCK, 0, st>>>(nr, d_rows + coff[c], N, d_indptr, d_indices, A, d_mask, x, b, sym ? 1 : 0);
        });
        if (launches) ++*launches;
    }
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

} // namespace igx
