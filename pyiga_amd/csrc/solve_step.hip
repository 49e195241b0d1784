// Parabolic problems on the device: DIRK time stepping of  M u' = f - K u  on the free dofs, u = g on the fixed ones
// (igx_solver_create_parabolic .. igx_solver_dirk_run; pyiga/solvers.py:366-473).  Every implicit stage
// solves  R C R^T y = R (b_i - C ext(g)),  C = M + tau gamma K,  with  b_i = M x + tau sum_{j<i} a_ij F_j + tau gamma f  and
// F_j = f - K y_j.
// Adaptive steps and Rosenbrock methods: a session of attempts (igx_solver_set_stepper .. igx_solver_error_ratio_d; DESIGN.md
// section 18; pyiga/solvers.py:430-435, 475-534, 684-707).  The host drives the controller; one attempt runs wholly on the
// device and leaves a candidate beside the untouched state.
// Kernels of its own: k_vals_axpby forms C, k_dirk_rhs the stage right-hand sides, k_err_norm the error estimate with its
// weighted norm, k_kron_lam the eigenvalue slots of the Kronecker factors for a new tau gamma.  The SpMVs, the stage solves and
// the preconditioners are those of solve.hip, reached through solve_internal.h.
#include "solve_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace igx;

namespace {

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

// the eigenvalue slots of the packed fast-diagonalization factors from the raw eigenvalues (LamSlots, solve_internal.h)
__global__ void k_kron_lam(const LamSlots L, const double *__restrict__ raw, double *fac, double scale, double shift)
{
    for (int k = 0; k < L.nax; ++k)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.m[k]; i += gridDim.x * blockDim.x)
            fac[L.slot[k] + i] = scale * raw[L.raw[k] + i] + shift;
}

// ---------------------------------------------------------------------------------------------
// DIRK time stepping

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
    if (s->par.d_dirk) return IGX_OK;
    const size_t nbytes = (size_t)s->n * sizeof(double);
    if (hipMalloc((void **)&s->par.d_dirk, (4 + IGX_DIRK_MAX_STAGES) * nbytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: out of device memory (%.3f GB)", what, (4.0 + IGX_DIRK_MAX_STAGES) * nbytes / 1e9);
        return IGX_ERR_NOMEM;
    }
    return IGX_OK;
}

// the buffer of C and the events of the time stepping (once)
int alloc_stage_matrix(igx_solver *s, const char *what)
{
    const long long nv = s->par.nvals[0];
    if (!s->par.pv[2]) {
        if (hipMalloc((void **)&s->par.pv[2], (size_t)nv * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: out of device memory (%.3f GB for C)", what, 8.0 * nv / 1e9);
            return IGX_ERR_NOMEM;
        }
    }
    if (!s->par.have_dev) {
        for (auto &e : s->par.dev)
            if (hipEventCreate(&e) != hipSuccess) { set_error("%s: hipEventCreate failed", what); return IGX_ERR_HIP; }
        s->par.have_dev = true;
    }
    return IGX_OK;
}

// C = M + tg K into the solver's buffer (k_vals_axpby between the events dev[0] and dev[1]; not synchronised)
int form_stage_matrix(hipStream_t st, igx_solver *s, double tg)
{
    const long long nv = s->par.nvals[0];
    const long long blocks = std::min<long long>((nv / 2 + BLOCK - 1) / BLOCK, 16LL * std::max(1, s->ctx->ncu));
    IGX_HIP(hipEventRecord(s->par.dev[0], st));
    k_vals_axpby<<<(unsigned)std::max<long long>(1, blocks), BLOCK, 0, st>>>(nv, 1.0, s->par.pv[0], tg, s->par.pv[1], s->par.pv[2]);
    IGX_HIP(hipGetLastError());
    IGX_HIP(hipEventRecord(s->par.dev[1], st));
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
    const unsigned nbv = vec_blocks(n);
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
        mask_copy(st, s, yprev, s->x);                                  // the initial guess y_{i-1}
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
            if (int rc = spmv_values(st, s, s->par.pv[1], c.y, c.fv, -1.0, c.F[i])) return rc;
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
    if (int rc = refuse_multipatch_block(s, what)) return rc;
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    if (role != IGX_ROLE_MASS && role != IGX_ROLE_OPERATOR) { set_error("%s: unknown role %d", what, role); return IGX_ERR_ARG; }
    if (s->par.pv[role]) { set_error("%s: role %d was taken already", what, role); return IGX_ERR_ARG; }
    igx_patch *pt = s->pt;
    const int kind = role == IGX_ROLE_MASS ? IGX_MASS : s->kind;
    if (pt->values_kind != kind || !pt->d_data) {
        set_error("%s: the patch holds no values of kind %d: assemble them first (igx_assemble, data_out may be NULL)", what, kind);
        return IGX_ERR_ARG;
    }
    const int other = 1 - role;
    if (s->par.pv[other] && s->par.nvals[other] != pt->nnz) {
        set_error("%s: value buffers of unequal length (%lld and %lld)", what, (long long)pt->nnz, s->par.nvals[other]);
        return IGX_ERR_ARG;
    }
    IGX_HIP(hipSetDevice(s->ctx->device));
    IGX_HIP(hipStreamSynchronize(pt->ctx->stream));
    s->par.pv[role] = pt->d_data;                       // the buffer changes hands: the patch's next assembly allocates anew
    s->par.nvals[role] = pt->nnz;
    pt->d_data = nullptr;
    pt->values_kind = -1;
    return IGX_OK;
}

int igx_solver_set_dirk(igx_solver *s, int stages, const double *A, double tau)
{
    const char *what = "igx_solver_set_dirk";
    if (!s || !A) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (int rc = refuse_multipatch_block(s, what)) return rc;
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    if (!s->par.pv[IGX_ROLE_MASS] || !s->par.pv[IGX_ROLE_OPERATOR]) { set_error("%s: take M and K first (igx_solver_take_values)", what); return IGX_ERR_ARG; }
    double gamma = 0.0;
    if (!dirk_ok(stages, A, tau, gamma, what)) return IGX_ERR_ARG;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (int rc = alloc_stage_matrix(s, what)) return rc;
    s->par.c_formed = false;
    s->precond = IGX_PRECOND_NONE;                   // (Jacobi's diagonal and the Kronecker factors depend on C: set them again)
    s->step.pc_vals = -1;
    if (int rc = form_stage_matrix(st, s, tau * gamma)) return rc;
    IGX_HIP(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&s->par.axpby_ms, s->par.dev[0], s->par.dev[1]);
    s->par.stages = stages;
    std::copy(A, A + (stages + 1) * stages, s->par.dirk_A);
    s->par.tau = tau;
    s->par.gamma = gamma;
    s->par.c_tg = tau * gamma;
    s->par.c_formed = true;
    return IGX_OK;
}

// Not built on the session calls (igx_solver_step_*), and dirk_A / tau / gamma not merged with st_*: the session scales the Kronecker
// eigenvalues on the device and stops its stage solves relative to the increment, so the iteration counts would change.
int igx_solver_dirk_run(igx_solver *s, const double *f, const double *gvals, const double *x0, int64_t nsteps, int64_t save_every,
                        double tol, int maxiter, int check_every, int timed, double *saved, int32_t *stage_iters, igx_dirk_info *info)
{
    const char *what = "igx_solver_dirk_run";
    if (!s || !f || (!gvals && !s->fixed.empty()) || !x0 || !saved) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (int rc = refuse_multipatch_block(s, what)) return rc;
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    if (nsteps < 1 || save_every < 1) { set_error("%s: nsteps and save_every must be >= 1", what); return IGX_ERR_ARG; }
    if (!(tol >= 0.0) || maxiter < 0) { set_error("%s: tol must be >= 0 and maxiter >= 0", what); return IGX_ERR_ARG; }
    if (int rc = check_values(s, what)) return rc;
    if (s->par.c_tg != s->par.tau * s->par.gamma || s->step.pc_vals != -1) {
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
    s->step.step_live = false;                                            // (the vectors of a stepping session are overwritten)
    double *xs = s->par.d_dirk, *mx = xs + n, *fv = xs + 2 * n, *y = xs + 3 * n, *F[IGX_DIRK_MAX_STAGES];
    for (int j = 0; j < IGX_DIRK_MAX_STAGES; ++j) F[j] = xs + (4 + j) * n;
    const int ns = s->par.stages;
    const double *A = s->par.dirk_A, tau = s->par.tau, gamma = s->par.gamma;
    const bool explicit_first = A[0] == 0.0;
    igx_dirk_info inf{};
    inf.axpby_ms = s->par.axpby_ms;
    s->bicg.breakdown = 0;
    hipEvent_t *E = s->par.dev;
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
        if (int rc = spmv_values(st, s, s->par.pv[1], xs, fv, -1.0, F[0])) return rc;
        if (int rc = T.lap(st, inf.spmv_ms)) return rc;
    }
    bool ok = true;
    long long last_saved = 0;
    for (long long k = 1; k <= nsteps && ok; ++k) {
        if (int rc = spmv_values(st, s, s->par.pv[0], xs, nullptr, 1.0, mx)) return rc;          // M x
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
// Adaptive steps and Rosenbrock methods: the session of attempts
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
// Kronecker factors (k_kron_lam) or Jacobi's diagonal (jacobi_diagonal on the values in use); nothing if they are in place
int step_refresh_precond(hipStream_t st, igx_solver *s, int which, double tg)
{
    s->precond = s->step.step_precond;
    if (s->step.pc_vals == which && (which == 0 || s->step.pc_tg == tg)) return IGX_OK;
    if (s->step.step_precond == IGX_PRECOND_KRON) {
        k_kron_lam<<<1, 256, 0, st>>>(s->step.lam_slots, s->step.d_lamraw, s->d_kron, which == 0 ? 0.0 : tg, 1.0 / s->dim);
        IGX_HIP(hipGetLastError());
    } else if (s->step.step_precond == IGX_PRECOND_JACOBI) {
        jacobi_diagonal(st, s, patch_values(s), s->dinv);
        IGX_HIP(hipGetLastError());
    }
    s->step.pc_vals = which;
    s->step.pc_tg = tg;
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
    return sum_partials(st, s, nbv, sum);                           // (k_fin in its fixed order; synchronised)
}

int step_solver_ok(const igx_solver *s, const char *what)
{
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (int rc = refuse_multipatch_block(s, what)) return rc;
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    if (!s->par.pv[IGX_ROLE_MASS] || !s->par.pv[IGX_ROLE_OPERATOR]) { set_error("%s: take M and K first (igx_solver_take_values)", what); return IGX_ERR_ARG; }
    return IGX_OK;
}

} // namespace

extern "C" {

int igx_solver_set_stepper(igx_solver *s, int family, int stages, const double *A, const double *Gamma, const double *b,
                           const double *b_hat)
{
    const char *what = "igx_solver_set_stepper";
    if (!s || !A) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (int rc = refuse_multipatch_block(s, what)) return rc;
    if (!s->parabolic) { set_error("%s: not a parabolic solver (igx_solver_create_parabolic)", what); return IGX_ERR_ARG; }
    double gamma = 0.0;
    if (family == IGX_STEPPER_DIRK) {
        if (Gamma) { set_error("%s: a DIRK scheme has no Gamma", what); return IGX_ERR_ARG; }
        if (!dirk_ok(stages, A, 1.0, gamma, what)) return IGX_ERR_ARG;
        for (int j = 0; j < stages; ++j) {
            if (b && b[j] != A[stages * stages + j]) { set_error("%s: b differs from the last row of A at %d", what, j); return IGX_ERR_ARG; }
            if (b_hat && !std::isfinite(b_hat[j])) { set_error("%s: b_hat[%d] is not finite", what, j); return IGX_ERR_ARG; }
        }
        std::copy(A, A + (stages + 1) * stages, s->step.st_A);
        std::copy(A + stages * stages, A + (stages + 1) * stages, s->step.st_b);
    } else if (family == IGX_STEPPER_ROSENBROCK) {
        if (!Gamma || !b) { set_error("%s: a Rosenbrock scheme needs Gamma and b", what); return IGX_ERR_ARG; }
        if (!rosenbrock_ok(stages, A, Gamma, b, b_hat, gamma, what)) return IGX_ERR_ARG;
        std::copy(A, A + stages * stages, s->step.st_A);
        std::copy(Gamma, Gamma + stages * stages, s->step.st_G);
        std::copy(b, b + stages, s->step.st_b);
    } else { set_error("%s: unknown family %d", what, family); return IGX_ERR_ARG; }
    s->step.st_bhat = b_hat != nullptr;
    if (b_hat) std::copy(b_hat, b_hat + stages, s->step.st_bh);
    s->step.family = family;
    s->step.st_stages = stages;
    s->step.st_gamma = gamma;
    s->step.step_live = false;                                 // (a session belongs to its scheme: begin again)
    return IGX_OK;
}

int igx_solver_set_step_precond(igx_solver *s, int precond, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                                const double *const *lam_raw)
{
    const char *what = "igx_solver_set_step_precond";
    if (int rc = step_solver_ok(s, what)) return rc;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    s->step.step_precond = -1;
    s->step.pc_vals = -1;
    if (precond == IGX_PRECOND_NONE || precond == IGX_PRECOND_JACOBI) { s->step.step_precond = precond; return IGX_OK; }
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
    if (int rc = upload_replacing(st, raw, s->step.d_lamraw)) return rc;
    s->kron = box_fastdiag(s, 0, box_lo, nb, s->d_kron, IGX_KRON_SUM);
    s->step.lam_slots = L;
    IGX_HIP(hipStreamSynchronize(st));
    s->step.step_precond = IGX_PRECOND_KRON;
    return IGX_OK;
}

int igx_solver_step_begin(igx_solver *s, const double *f, const double *gvals, const double *x0)
{
    const char *what = "igx_solver_step_begin";
    if (int rc = step_solver_ok(s, what)) return rc;
    if (!f || (!gvals && !s->fixed.empty()) || !x0) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (s->step.family < 0) { set_error("%s: no scheme yet (igx_solver_set_stepper)", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const long long n = s->n;
    const size_t nbytes = (size_t)n * sizeof(double);
    s->step.step_live = false;
    if (int rc = alloc_dirk_vectors(s, what)) return rc;
    if (int rc = alloc_stage_matrix(s, what)) return rc;
    if (!s->step.d_wg) {
        if (hipMalloc((void **)&s->step.d_wg, nbytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: out of device memory (%.3f GB)", what, nbytes / 1e9);
            return IGX_ERR_NOMEM;
        }
    }
    double *v = s->par.d_dirk;
    s->step.sx = v; s->step.smx = v + n; s->step.sfv = v + 2 * n; s->step.sy = v + 3 * n;
    for (int j = 0; j < IGX_DIRK_MAX_STAGES; ++j) s->step.sF[j] = v + (4 + j) * n;
    if (int rc = upload_start_state(st, s, f, gvals, x0, s->step.sx, s->step.d_wg, s->step.sfv, nullptr)) return rc;
    s->step.have_mx = s->step.have_F0 = s->step.have_cand = false;
    s->bicg.breakdown = 0;
    s->step.step_live = true;
    return IGX_OK;
}

int igx_solver_step_attempt(igx_solver *s, double tau, double err_tol, double solve_tol, int maxiter, int check_every, int timed,
                            igx_step_info *info)
{
    const char *what = "igx_solver_step_attempt";
    if (int rc = step_solver_ok(s, what)) return rc;
    if (!s->step.step_live) { set_error("%s: no session (igx_solver_step_begin; igx_solver_dirk_run and igx_solver_set_stepper end one)", what); return IGX_ERR_ARG; }
    if (s->step.step_precond < 0) { set_error("%s: no preconditioner of the session (igx_solver_set_step_precond; igx_solver_set_precond replaces it)", what); return IGX_ERR_ARG; }
    if (!(tau > 0.0) || !std::isfinite(tau)) { set_error("%s: tau must be positive and finite", what); return IGX_ERR_ARG; }
    if (!(solve_tol >= 0.0) || maxiter < 0) { set_error("%s: solve_tol must be >= 0 and maxiter >= 0", what); return IGX_ERR_ARG; }
    if (err_tol > 0.0 && !s->step.st_bhat) { set_error("%s: the scheme has no embedded rule (b_hat): err_tol must be <= 0", what); return IGX_ERR_ARG; }
    if (check_every < 1) check_every = 1;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const long long n = s->n;
    const int ns = s->step.st_stages;
    const double *A = s->step.st_A, gamma = s->step.st_gamma, tg = tau * gamma;
    const bool estimate = err_tol > 0.0;
    const unsigned nbv = vec_blocks(n);
    igx_step_info inf{};
    inf.n_free = n - (long long)s->fixed.size();
    inf.has_estimate = estimate ? 1 : 0;
    s->step.have_cand = false;
    s->bicg.breakdown = 0;
    s->par.vals_sel = nullptr;
    hipEvent_t *E = s->par.dev;
    IGX_HIP(hipEventRecord(E[4], st));
    if (!s->par.c_formed || s->par.c_tg != tg) {                            // C on the device belongs to another step
        s->par.c_formed = false;
        if (int rc = form_stage_matrix(st, s, tg)) return rc;
        IGX_HIP(hipEventSynchronize(E[1]));
        (void)hipEventElapsedTime(&s->par.axpby_ms, E[0], E[1]);
        inf.axpby_ms = s->par.axpby_ms;
        inf.reformed = 1;
        s->par.c_tg = tg;
        s->par.c_formed = true;
        s->step.pc_vals = -1;
    }
    if (int rc = step_refresh_precond(st, s, 2, tg)) return rc;
    PhaseTimer T{E, 2, 3, timed};                                    // (E[0], E[1]: k_vals_axpby)
    if (timed) IGX_HIP(hipEventRecord(E[2], st));
    bool ok = true;
    double sum = 0.0;
    if (s->step.family == IGX_STEPPER_DIRK) {
        double *xs = s->step.sx, *mx = s->step.smx, *fv = s->step.sfv, *y = s->step.sy, **F = s->step.sF;
        const bool explicit_first = A[0] == 0.0;
        if (explicit_first && !s->step.have_F0) {                         // F_1 of the first step: f - K x0
            if (int rc = spmv_values(st, s, s->par.pv[1], xs, fv, -1.0, F[0])) return rc;
            s->step.have_F0 = true;
        }
        if (!s->step.have_mx) {                                           // M x: kept over rejected attempts
            if (int rc = spmv_values(st, s, s->par.pv[0], xs, nullptr, 1.0, mx)) return rc;
            s->step.have_mx = true;
        }
        if (int rc = T.lap(st, inf.spmv_ms)) return rc;
        // the stage solves stop relative to the increment; the last F as F_1 of the next step, or where the embedded rule weighs it
        const bool have_Fs = explicit_first || (estimate && s->step.st_bh[ns - 1] != s->step.st_b[ns - 1]);
        const StageChain chain{A, ns, tau, tg, xs, mx, fv, y, F, s->step.d_wg, true, solve_tol, maxiter, check_every, have_Fs,
                               inf.stage_iterations, &inf.spmv_ms, &inf.combine_ms, &inf.solve_ms};
        if (int rc = dirk_stage_chain(st, s, chain, T, ok)) return rc;
        if (ok && estimate) {
            // e = x_est - x_new: the last stage equation is M x_new = M x + tau sum b_i F_i, so R M R^T e = tau sum (b^_i - b_i) F_i
            // (the F_i vanish on the fixed dofs; nothing to lift).  One CG solve on M from zero: its relative residual is that
            // of the estimate itself, not of the 1/err_tol times larger x_est
            Comb L{};
            for (int j = 0; j < ns; ++j) {
                const double c = s->step.st_bh[j] - s->step.st_b[j];
                if (c != 0.0 && (j < ns - 1 || have_Fs)) { L.c[L.nv] = tau * c; L.v[L.nv++] = F[j]; }
            }
            k_dirk_rhs<<<nbv, BLOCK, 0, st>>>(n, L, s->b);
            IGX_HIP(hipGetLastError());
            if (int rc = T.lap(st, inf.combine_ms)) return rc;
            s->par.vals_sel = s->par.pv[IGX_ROLE_MASS];
            const int method = s->method;
            s->method = IGX_METHOD_CG;                               // (M is symmetric positive definite whatever K is)
            igx_solve_info si{};
            int rc = step_refresh_precond(st, s, 0, 0.0);
            if (!rc) rc = solve_lifted(st, s, nullptr, false, solve_tol, maxiter, check_every, 0, si);
            s->method = method;
            s->par.vals_sel = nullptr;
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
        double *xs = s->step.sx, *cand = s->step.smx, *fv = s->step.sfv, *yt = s->step.sy, **K = s->step.sF;
        const double *G = s->step.st_G;
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
            if (int rc = spmv_values(st, s, s->par.pv[1], yi, fv, -1.0, s->b)) return rc;
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
                if (s->step.st_b[j] != 0.0) { L.c[L.nv] = tau * s->step.st_b[j]; L.v[L.nv++] = K[j]; }
            k_dirk_rhs<<<nbv, BLOCK, 0, st>>>(n, L, cand);
            IGX_HIP(hipGetLastError());
            if (int rc = T.lap(st, inf.combine_ms)) return rc;
            if (estimate) {
                Comb D{};
                for (int j = 0; j < ns; ++j) {
                    const double c = s->step.st_bh[j] - s->step.st_b[j];
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
    s->step.have_cand = ok;
    if (info) *info = inf;
    return IGX_OK;
}

int igx_solver_step_accept(igx_solver *s)
{
    const char *what = "igx_solver_step_accept";
    if (int rc = step_solver_ok(s, what)) return rc;
    if (!s->step.step_live || !s->step.have_cand) { set_error("%s: no candidate (a converged igx_solver_step_attempt first)", what); return IGX_ERR_ARG; }
    if (s->step.family == IGX_STEPPER_DIRK) {
        std::swap(s->step.sx, s->step.sy);                                     // x_new = y_s
        if (s->step.st_A[0] == 0.0) std::swap(s->step.sF[0], s->step.sF[s->step.st_stages - 1]);
    } else std::swap(s->step.sx, s->step.smx);
    s->step.have_mx = false;
    s->step.have_cand = false;
    return IGX_OK;
}

int igx_solver_step_state(igx_solver *s, int which, double *out)
{
    const char *what = "igx_solver_step_state";
    if (int rc = step_solver_ok(s, what)) return rc;
    if (!out) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->step.step_live) { set_error("%s: no session (igx_solver_step_begin)", what); return IGX_ERR_ARG; }
    if (which != IGX_STEP_STATE && which != IGX_STEP_CANDIDATE) { set_error("%s: unknown vector %d", what, which); return IGX_ERR_ARG; }
    if (which == IGX_STEP_CANDIDATE && !s->step.have_cand) { set_error("%s: no candidate (a converged igx_solver_step_attempt first)", what); return IGX_ERR_ARG; }
    const double *src = which == IGX_STEP_STATE ? s->step.sx : s->step.family == IGX_STEPPER_DIRK ? s->step.sy : s->step.smx;
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
