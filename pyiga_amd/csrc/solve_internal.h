// What the units of the device solvers know of each other: solve.hip (the linear solvers, the block solver, Newton's method),
// solve_step.hip (DIRK time stepping and the adaptive stepping session), solve_eig.hip (the block eigen-solver), solve_saddle.hip
// (saddle-point systems, MINRES) and solve_gmres.hip (GMRES on them).  It holds
// what more than one of them needs and nothing else: the solver structure with the state of every mode in a group of its own,
// the layout types and device helpers the row kernels of two units share, and the host helpers that cross a unit boundary.  A
// kernel is launched only from the unit that defines it; a kernel that another unit needs has a host function here.
// (multigrid.hip keeps its narrower view of a solver: mg_internal.h.)
#pragma once
#include "igx_internal.h"
#include "mg_internal.h"

#include <vector>

namespace igx {

constexpr int BLOCK = 256;
constexpr int NB_VEC = 1024;             // blocks of the vector kernels (and most partial sums of a dot product)
constexpr int NB_SPMV_MAX = 8192;        // blocks of the SpMV (grid-stride over rows): what is resident at once, at most this

typedef double dbl2 __attribute__((ext_vector_type(2)));

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

// the NC x NC blocks of a vector-valued form: v[p * NC + q] holds block (p, q) (test component p, trial component q) in the
// patch's structured layout (a multipatch block solver: in the order of the multipatch's global CSR pattern), or is null (a
// block that was never assembled: zero)
struct BlockVals {
    const double *v[9];
};

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

// the fast-diagonalization inverse  (x) U_k . D^-1 . (x) U_k^T  of one box (m[k] dofs on axis k): x is read and y written at
// io_off with the strides io_stride, in between compact box vectors.  Its factors, per axis U_k^T | U_k | lam_k, lie in one
// device buffer (pack_fastdiag).
struct FastDiag {
    int dim;
    KronPlan kl, kr;                     // (x) U_k^T with D^-1, then (x) U_k
};

// the box of one patch in its local dofs (3D; a 2D patch has a one-dof outer axis) and its local-to-global map
struct BoxMap {
    int lo[3], nb[3], N[3];
    long long nbox;
    const int32_t *l2g;
};

// one patch of the Schwarz preconditioner: its box and its fast-diagonalization inverse (compact box vectors in and out)
struct SwPatch {
    BoxMap map;
    FastDiag F;
};

// the eigenvalue slots of the packed fast-diagonalization factors from the raw eigenvalues kept beside them:
// lam'_k = scale lam_k + shift  (C = M + tau gamma K: scale = tau gamma, shift = 1/dim; M: scale = 0)
struct LamSlots {
    int nax;
    int m[3];
    long long slot[3], raw[3];               // offsets of lam'_k in the factor buffer and of lam_k in the raw one
};

// ---------------------------------------------------------------------------------------------
// The state of each mode of a solver.  release() frees the group's device memory and events (once, when the solver goes).

// BiCGStab (allocated only once a solver is switched to it): v = q, p^ = z; r^ | s | s^ | t in d_bvec, its scalars in d_bsc
struct BicgState {
    double *d_bvec = nullptr;
    double *rh = nullptr, *sv = nullptr, *sh = nullptr, *t = nullptr;
    double *d_bsc = nullptr;
    int breakdown = 0;                        // reason of the last BiCGStab solve (IGX_BREAKDOWN_*), 0 if none
    hipEvent_t bev[8] = {};
    bool have_bev = false;
    void release()
    {
        (void)hipFree(d_bvec); (void)hipFree(d_bsc);
        if (have_bev)
            for (auto &e : bev) (void)hipEventDestroy(e);
    }
};

// block solver of a vector-valued form (igx_solver_create_block): ncomp components of g.nrows dofs each, n = ncomp g.nrows
struct BlockState {
    double *blk[9] = {};                      // block (p, q) at p * ncomp + q, taken from the patch (owned), or null
    bool hidden[9] = {};                      // a saddle solver's products leave the block out (igx_solver_hide_block); it stays owned
    FastDiag bkron[3] = {};                   // per component: the fast-diagonalization inverse on its free box (in d_bkron[c])
    double *d_bkron[3] = {};
    int klo[3][3] = {}, knb[3][3] = {}, kmode[3] = {};   // per component: its box and lam_mode (the eigen-solver's batched plans)
    double *mass = nullptr;                   // the scalar mass matrix of the eigen-solver (igx_solver_take_mass), owned, or null
    // a multipatch block solver (igx_solver_create_multipatch_block): blk[] are copies of the multipatch's sums (nnz values each),
    // and per component the Schwarz patches of igx_solver_set_block_schwarz, whose packed factors lie in d_bkron[c]
    std::vector<SwPatch> bsw[3];
    void release()
    {
        for (double *v : blk) (void)hipFree(v);
        for (double *v : d_bkron) (void)hipFree(v);
        (void)hipFree(mass);
    }
};

// parabolic solver (igx_solver_create_parabolic): M and K taken from the patch (IGX_ROLE_*), C = M + tau gamma K formed by
// igx_solver_set_dirk; the SpMV, Jacobi and the solves act on C
struct ParState {
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
    double c_tg = 0.0;                        // the tau gamma of the C on the device (c_formed)
    const double *vals_sel = nullptr;         // the values the SpMV and Jacobi read instead of C (the mass solve: M)
    void release()
    {
        for (double *v : pv) (void)hipFree(v);
        (void)hipFree(d_dirk);
        if (have_dev)
            for (auto &e : dev) (void)hipEventDestroy(e);
    }
};

// adaptive stepping session (igx_solver_set_stepper .. igx_solver_step_accept)
struct StepState {
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
    double *sx = nullptr, *smx = nullptr, *sfv = nullptr, *sy = nullptr, *sF[IGX_DIRK_MAX_STAGES] = {};     // (in par.d_dirk)
    void release() { (void)hipFree(d_lamraw); (void)hipFree(d_wg); }
};

struct EigState;                              // the session of the block eigen-solver (solve_eig.hip)

// per-axis tables of a rectangular value layout (the matrix of a pair, or its transpose), as a 3D layout like Geom: row
// (i0, i1, i2) of the space N holds the columns prod_k [lo_k[i_k], hi_k[i_k]) of the space M in lexicographic order
struct RectGeom {
    int N[3], M[3];
    const int *lo[3], *hi[3], *rp[3];
    long long S1, S2;
    long long nrows;
};

// saddle-point solver (igx_solver_create_saddle, solve_saddle.hip): [[A, B^T], [B, 0]] with the blocks A_pq
// of the block solver (block.blk) over nu velocity dofs per component and B_q over np pressure dofs; n = ncomp nu + np
struct SaddleState {
    const igx_pair *pair = nullptr;           // the pair the solver was made over (its tables were copied: identity only)
    long long nu = 0, np = 0, nnzB = 0;
    int Np[3] = {1, 1, 1};                    // pressure dofs per axis (dim of them)
    double *B[3] = {}, *BT[3] = {};           // B_q (taken from the pair, owned) and B_q^T in the layout of the swapped spaces
    int *d_rtab = nullptr;                    // the tables of gB and gT
    RectGeom gB{}, gT{};
    int gw_u = 4, gw_p = 4, nb_u = 1, nb_p = 1;       // group width and resident blocks of each row kernel (fixed per solver)
    int schur = -1;                           // the pressure part of the preconditioner: IGX_PRECOND_JACOBI / _KRON, -1: not set
    FastDiag skron{};
    double *d_skron = nullptr, *d_sdinv = nullptr;
    double sscale = 1.0;
    long long swlen = 0;                      // the pressure box of skron (the work buffers d_W hold two of the largest box)
    double *d_mvec = nullptr;                 // MINRES: r1 | r2 | y | v | w | w1 | w2, n each (allocated with the solver)
    double *d_msc = nullptr;                  // its scalars (MS_*), written by k_fin_minres only
    int breakdown = 0;                        // IGX_BREAKDOWN_* of the last solve
    int project = 0;                          // the solves remove the mean of the pressure part of the lifted right-hand side
    double rhs_mean = 0.0, rhs_norm = 0.0;    // of that pressure part at the last solve
    long long maxT = 1;                       // longest row of B^T
    // device times (igx_solver_saddle_timing): of the last k_pair_transpose, and of the velocity- and the pressure-row launch of
    // the last igx_solver_saddle_product_d
    float transpose_ms = 0.0f, u_ms = 0.0f, p_ms = 0.0f;
    void release()
    {
        for (double *v : B) (void)hipFree(v);
        for (double *v : BT) (void)hipFree(v);
        (void)hipFree(d_rtab); (void)hipFree(d_skron); (void)hipFree(d_sdinv); (void)hipFree(d_mvec); (void)hipFree(d_msc);
    }
};

// restarted GMRES on a saddle-point solver (igx_solver_set_gmres, solve_gmres.hip).  Its work vectors are
// the MINRES ones (sad.d_mvec: rhs | z | t | the triangular preconditioner's velocity right-hand side), which a GMRES solve
// leaves free
struct GmresState {
    int restart = 0;                          // 0: the solver solves with MINRES
    int triangular = 0;                       // the block upper-triangular preconditioner (saddle_apply_precond)
    int cap = 0;                              // the restart the arrays below were allocated for
    double *d_V = nullptr;                    // the basis: (cap + 1) columns of n
    double *d_small = nullptr;                // scalars | h | hp | cs | sn | g | y | R (gmres_small_len(cap) doubles)
    int project_ops = 0;                      // the solve runs on Q K Q and Q P, Q taking the pressure mean off (igx_solver_saddle_correct_d
                                              // on a projecting solver: DESIGN.md section 33); 0: the operators as they are
    int restarts = 0;                         // of the last solve
    float orth_ms = 0.0f, combine_ms = 0.0f;  // device time of the orthogonalisations / the updates of x of the last timed solve
                                              // (igx_solver_gmres_orth_d, _combine_d: of that call)
    int orth_count = 0, combine_count = 0;    // how many of each those times cover
    void release() { (void)hipFree(d_V); (void)hipFree(d_small); }
};

} // namespace igx

struct igx_solver {
    igx_ctx *ctx = nullptr;
    igx_patch *pt = nullptr;                  // the patch of a patch solver, or
    igx_multipatch *mp = nullptr;             // the global sums of a multipatch solver
    unsigned long long gen = 0;               // mp->generation the solver was made over
    int kind = 0;
    int dim = 0;
    int N[3] = {1, 1, 1};                    // dofs per axis of the patch (dim of them)
    long long n = 0;
    igx::Geom g{};
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
    igx::FastDiag kron{};                     // the Kronecker preconditioner on the free box of the full-length vectors
    double *d_kron = nullptr;                 // U_k^T | U_k | lam_k (Schwarz: of every patch)
    double *d_W = nullptr;                    // two work buffers
    long long wlen = 0;
    std::vector<igx::SwPatch> sw;             // Schwarz: the patches with a non-empty box
    double *d_box = nullptr;                  // Schwarz: one patch's box (gathered residual, then the local correction)
    hipEvent_t ev[6] = {};
    bool have_ev = false;
    int method = IGX_METHOD_CG;
    int ncomp = 1;                            // components of a block solver (1: scalar); with mp set: a multipatch block solver
    bool symmetric = false;                   // made as symmetric: CG allowed
    bool parabolic = false;
    igx::BicgState bicg;
    igx::BlockState block;
    igx::ParState par;
    igx::StepState step;
    // multigrid (igx_solver_set_mg_*, multigrid.hip): this solver's level of the hierarchy, or null
    igx::MgLevel *mg = nullptr;
    // block eigen-solver (igx_solver_eig_*, solve_eig.hip): made by its first call, or null
    igx::EigState *eig = nullptr;
    double *d_mass = nullptr;                 // a multipatch solver's second matrix (igx_solver_set_mass_d), owned
    bool saddle = false;                      // made by igx_solver_create_saddle: n = ncomp g.nrows + sad.np, MINRES or GMRES (gm)
    igx::SaddleState sad;
    igx::GmresState gm;
};

namespace igx {

// ---- solve.hip
int check_values(const igx_solver *s, const char *what);
const double *patch_values(const igx_solver *s);
unsigned vec_blocks(long long n);
int spmv(hipStream_t st, const igx_solver *s, const double *x, const double *b, double sign, double *y, const double *pd, double *part);
int spmv_values(hipStream_t st, const igx_solver *s, const double *vals, const double *x, const double *b, double sign, double *y);
int solve_lifted(hipStream_t st, igx_solver *s, const double *lift, bool x0_in_x, double tol, int maxiter, int check_every, int timed,
                 igx_solve_info &inf, bool from_guess = false);
int apply_fastdiag(hipStream_t st, const FastDiag &F, const double *x, double *y, double *const W[2]);
// (dims: the dofs per axis of the space the box lies in, default the patch's s->N; a box that need not be the free dofs: free_is_box
// false -- the caller masks what the inverse returns)
int box_fastdiag_setup(igx_solver *s, long long base, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                       const double *const *lam, int lam_mode, const char *what, int *reset, double *&d_fac, int nb[3],
                       const int *dims = nullptr, bool free_is_box = true);
FastDiag box_fastdiag(const igx_solver *s, long long base, const int32_t *box_lo, const int *nb, const double *d_fac, int lam_mode,
                      long long batch = 1, const int *dims = nullptr);
int alloc_fastdiag_work(igx_solver *s, long long wlen);
int upload_replacing(hipStream_t st, const std::vector<double> &h, double *&d_buf);
bool create_args_ok(const void *owner, const int64_t *fixed, int64_t nfixed, igx_solver **out, const char *what);
// (extra: entries of the vectors past the ncomp components of the patch -- the pressure dofs of a saddle solver)
int create_patch_solver(igx_patch *pt, int kind, int ncomp, bool values_now, const int64_t *fixed, int64_t nfixed, igx_solver **out,
                        const char *what, long long extra = 0);
int init_bicgstab(igx_solver *s, const char *what);
void free_solver(igx_solver *s);
int close_call(hipStream_t st, hipEvent_t begin, hipEvent_t end, const char *what, float &total_ms);
// IGX_ERR_UNSUPPORTED (with igx_last_error) if s is a multipatch block solver, which serves the linear solves only; else IGX_OK
int refuse_multipatch_block(const igx_solver *s, const char *what);
// the kernels of solve.hip that the other units need, each behind the one launch its callers made (not synchronised; a launch
// failure shows in the caller's hipGetLastError)
void mask_copy(hipStream_t st, const igx_solver *s, const double *x, double *y);          // k_mask_copy: y = free ? x : 0
// k_diag / k_csr_diag: dinv = free ? 1 / diag(A) : 0 for the matrix `vals` in the solver's layout (a multipatch's CSR pattern, else
// the patch's structured one; a block solver of either layout: the diagonal block of component comp, whose rows of the mask
// start at comp times the scalar rows; dinv points at the component's slice)
void jacobi_diagonal(hipStream_t st, const igx_solver *s, const double *vals, double *dinv, int comp = 0);
// k_fin: the first nb partial sums of s->d_part added up in their fixed order, read back into *sum (synchronised)
int sum_partials(hipStream_t st, igx_solver *s, unsigned nb, double *sum);

int spmv_group_width(long long maxlen);       // spmv_gw: the group width of the row kernels for a longest row of maxlen entries

// ---- solve_saddle.hip
// IGX_ERR_UNSUPPORTED (with igx_last_error) if s is a saddle-point solver, which serves MINRES solves, the product and its
// preconditioner only; else IGX_OK
int refuse_saddle(const igx_solver *s, const char *what);
int saddle_check_values(const igx_solver *s, const char *what);
int saddle_spmv(hipStream_t st, const igx_solver *s, const double *x, const double *b, double sign, double *y, const double *pd, double *part,
                hipEvent_t mid = nullptr);
int saddle_set_precond(igx_solver *s, int precond);
int saddle_apply_precond(hipStream_t st, igx_solver *s, const double *r, double *z);
int saddle_solve_lifted(hipStream_t st, igx_solver *s, const double *lift, bool x0_in_x, double tol, int maxiter, int check_every, int timed,
                        igx_solve_info &inf);

// the mean of the free pressure part of v taken off it (a projecting solver; else nothing changes)
int saddle_project_vector(hipStream_t st, igx_solver *s, double *v);

// y = a + b over the n entries (k_mr_add)
void saddle_add(hipStream_t st, long long n, const double *a, const double *b, double *y);

// ---- solve_gmres.hip
// Right-preconditioned GMRES(s->gm.restart) on R K R^T x = rhs: the residual rhs - K x0 in s->r, x0 in s->x, rhs itself in `rhs`
// (s->r where x0 = 0).  What solve_minres is to a solver with gm.restart == 0: saddle_solve_lifted enters one or the other.
int solve_gmres(hipStream_t st, igx_solver *s, const double *rhs, double tol, int maxiter, int check_every, int timed, igx_solve_info &inf);

// ---- solve_eig.hip
void eig_free(igx_solver *s);                // the eigen-solver's state and the mass matrix of a multipatch solver
void eig_drop_block_kron(igx_solver *s);      // a block solver's Kronecker factors were replaced: the eigen pieces select them again

} // namespace igx
