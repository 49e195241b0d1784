// What solve.hip and multigrid.hip know of each other.  The solver structure stays private to solve.hip; the multigrid levels
// stay private to multigrid.hip, hung on the solver through one pointer.
#pragma once
#include "igx_internal.h"

namespace igx {

struct MgLevel;                               // the multigrid state of one solver (multigrid.hip)

// what the multigrid reads of a multipatch solver
struct SolverRef {
    igx_ctx *ctx;
    igx_multipatch *mp;                       // null: a patch solver
    long long n;
    int gw;                                   // group width of the solver's CSR SpMV
    const uint8_t *d_mask;                    // 1 on the free dofs (device), and
    const uint8_t *h_free;                    // the same on the host
    int precond, method;
    int ncomp;                                // > 1: a multipatch block solver (its hierarchy: igx_solver_set_block_mg_*)
    long long N;                              // scalar global dofs (nodes): n / ncomp
    const double *blk[9];                     // a block solver's block (p, q) at p * ncomp + q over the CSR pattern, or null (absent)
    bool symmetric;                           // a block solver made as symmetric
};

// solve.hip
SolverRef solver_ref(const igx_solver *s);
MgLevel *&solver_mg(igx_solver *s);
void solver_drop_mg_precond(igx_solver *s);   // IGX_PRECOND_MG -> IGX_PRECOND_NONE (a level of the hierarchy went away)
int solver_check_sums(const igx_solver *s, const char *what);      // IGX_ERR_ARG once the multipatch's sums were restarted
// y = free ? b - A x : 0 through the solver's SpMV dispatch
int solver_residual(hipStream_t st, const igx_solver *s, const double *x, const double *b, double *y);

// multigrid.hip
void mg_free(igx_solver *s);                  // the levels' device memory and the links to the neighbouring levels
int mg_check(const igx_solver *s, const char *what);               // the hierarchy below s is complete and every level's sums are current
int mg_apply(hipStream_t st, igx_solver *s, const double *r, double *z);   // z = one V-cycle on r (r zero on the fixed dofs)
// The launchers of the smoother and the dense coarse solve, for any CSR matrix on the device (hmg.hip uses them too).
// One Gauss-Seidel sweep over the rows d_rows, sorted by (colour, index); colour c holds rows coff[c] .. coff[c + 1] (coff on the
// host, d_coff its device copy).  one_block: k_csr_gs_block, all colours in one launch of one block; else k_csr_gs, one launch per
// colour.  backward: the colours in descending order.  *launches (may be null) is advanced by the launches made.
int csr_gs_sweep(hipStream_t st, int gw, int ncol, const int *coff, const int *d_coff, const int32_t *d_rows, bool one_block,
                 const int32_t *d_indptr, const int32_t *d_indices, const double *d_vals, double *x, const double *b, bool backward,
                 int *launches);
// multigrid_block.hip: one node-block Gauss-Seidel sweep (k_csr_node_gs, one launch per colour) over the nc x nc blocks blk of a
// multipatch block solver on the pattern of N scalar rows; d_rows lists the nodes with a free component by (colour, index),
// d_mask is the mask over the nc * N blocked dofs.  sym: the diagonal blocks' lower triangles are taken from the upper ones.
int csr_node_gs_sweep(hipStream_t st, int gw, int nc, int ncol, const int *coff, const int32_t *d_rows, long long N,
                      const int32_t *d_indptr, const int32_t *d_indices, const double *const *blk, const uint8_t *d_mask, bool sym,
                      double *x, const double *b, bool backward, int *launches);
// k_dense_apply: x[d_idx[i]] = sum_j d_inv[i][j] b[d_idx[j]], i < m
int dense_apply(hipStream_t st, int m, const double *d_inv, const int32_t *d_idx, const double *b, double *x);

} // namespace igx
