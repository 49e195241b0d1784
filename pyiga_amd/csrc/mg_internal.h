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
    int ncomp;                                // > 1: a multipatch block solver (no multigrid)
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

} // namespace igx
