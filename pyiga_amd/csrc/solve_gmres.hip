// Restarted GMRES on a saddle-point solver (igx_solver_set_gmres and the inspection calls igx_solver_gmres_orth_d,
// igx_solver_gmres_combine_d, igx_solver_gmres_timing, igx_solver_gmres_restarts; include/igx.h): the
// Krylov method of the Oseen systems  [[nu A + N(w), B^T], [B, 0]], whose velocity block is not symmetric.
//
// Right-preconditioned GMRES(m) on R K R^T x = rhs.  One Arnoldi step j: z = P v_j (saddle_apply_precond), v_{j+1} = K z
// (saddle_spmv, written straight into the next basis column), classical Gram-Schmidt twice against v_0 .. v_j in place, the
// scale by 1 / h_{j+1,j} in place.  The basis stays in HBM; the Hessenberg column, the Givens rotations, g and y live on the
// device and only k_gm_fin writes them; the host reads the scalars back every check_every steps and at the end of a cycle.
//   k_gm_dots<MB>    per-block partials of v_k . w for every column k, MB columns per pass over w (chunks walked in the kernel)
//   k_gm_update<MB>  w -= sum_k h_k v_k, w held in registers over the chunks; the second pass also emits the partials of w . w
//   k_gm_fin         one block: the partials summed in block order into h; the rotations, g, the stop; the back substitution
//   k_gm_scale       v = w / h_{j+1,j} (and v_0 = r / ||r||)
//   k_gm_combine<MB> t = sum_k y_k v_k; then x += P t (saddle_apply_precond and k_gm_axpy)
// After the stop (GS_LAST, then GS_DONE) every kernel returns at once: steps run past it (check_every > 1) change nothing.
#include "solve_internal.h"

#include <algorithm>
#include <cmath>

using namespace igx;

namespace {

constexpr int MB = 8;                    // basis columns per pass over w
constexpr int GM_MAX_RESTART = 128;
// d_part (2 NB_SPMV_MAX doubles) holds the partials of one orthogonalisation: those of k_gm_dots in front, gm_dot_blocks(n, m)
// blocks times at most m + 1 columns <= GM_DOT_PART, and behind them those of w . w of k_gm_update / k_gm_sumsq, one per block
// of vec_blocks(n) <= NB_VEC
constexpr int GM_DOT_PART = 2 * NB_SPMV_MAX - NB_VEC;

// the scalars (only k_gm_fin writes them).  GS_LAST: the step that met the stop; the update of x that follows is the final one,
// after which GS_DONE freezes everything.  A breakdown sets GS_DONE at once: x keeps the iterate of the last finished cycle.
enum { GS_IT = 0, GS_J, GS_DONE, GS_LAST, GS_CONV, GS_REASON, GS_STOP, GS_BETA, GS_HNEXT, GS_K, GS_RESTARTS, GS_N = 16 };
enum { GF_START = 0, GF_RESTART, GF_H1, GF_H2, GF_ROT, GF_NORM, GF_Y, GF_CLOSE };

// the small device arrays of a solver allocated for restart m, one after the other
struct Small {
    double *sc, *h, *hp, *cs, *sn, *g, *y, *R;
    int ld;                                        // leading dimension of R (column j: the rotated Hessenberg column of step j)
};

size_t small_len(int m) { return GS_N + 7 * (size_t)(m + 2) + (size_t)(m + 2) * (m + 2); }

Small small_of(double *p, int m)
{
    Small a;
    const int l = m + 2;
    a.sc = p; a.h = p + GS_N; a.hp = a.h + l; a.cs = a.hp + l; a.sn = a.cs + l; a.g = a.sn + l; a.y = a.g + l; a.R = a.y + l;
    a.ld = l;
    return a;
}

__device__ __forceinline__ bool gm_finite(double v)           // (the exponent-bit test of k_fin_minres)
{
    return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

__device__ __forceinline__ bool gm_stopped(const double *sc) { return sc[GS_DONE] != 0.0 || sc[GS_LAST] != 0.0; }

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the sum of v over the block in a fixed order (the waves' sums added one after the other); sh: BLOCK / 64 doubles
__device__ __forceinline__ double gm_block_sum(double v, double *sh)
{
    v = wave_sum(v);
    if (threadIdx.x % 64 == 0) sh[threadIdx.x / 64] = v;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int k = 1; k < BLOCK / 64; ++k) s += sh[k];
    __syncthreads();
    return s;
}

// part[block * c + k] = sum over the block's entries of V[k n + i] w[i], k < c
template <int M>
__global__ void __launch_bounds__(BLOCK) k_gm_dots(long long n, const double *__restrict__ V, int c, const double *__restrict__ w,
                                                   double *__restrict__ part, const double *__restrict__ sc)
{
    __shared__ double sh[BLOCK / 64][M];
    if (gm_stopped(sc)) return;
    const long long stride = (long long)gridDim.x * BLOCK;
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    for (int k0 = 0; k0 < c; k0 += M) {
        const int cnt = min(M, c - k0);
        const double *__restrict__ Vk = V + (long long)k0 * n;
        double acc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = 0.0;
        if (cnt == M) {
            for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
                const double wi = w[i];
                double v[M];
#pragma unroll
                for (int m = 0; m < M; ++m) v[m] = Vk[(long long)m * n + i];
#pragma unroll
                for (int m = 0; m < M; ++m) acc[m] += v[m] * wi;
            }
        } else {
            for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
                const double wi = w[i];
#pragma unroll
                for (int m = 0; m < M; ++m)
                    if (m < cnt) acc[m] += Vk[(long long)m * n + i] * wi;
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double v = wave_sum(acc[m]);
            if (lane == 0) sh[wave][m] = v;
        }
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            double s = sh[0][threadIdx.x];
#pragma unroll
            for (int k = 1; k < BLOCK / 64; ++k) s += sh[k][threadIdx.x];
            part[(long long)blockIdx.x * c + k0 + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

// w -= sum_{k < c} h[k] V[k n + i] in the order of k; partN[block] = sum of the new w^2 (optional)
template <int M>
__global__ void __launch_bounds__(BLOCK) k_gm_update(long long n, const double *__restrict__ V, int c, const double *__restrict__ h,
                                                     double *__restrict__ w, double *__restrict__ partN, const double *__restrict__ sc)
{
    __shared__ double sh[BLOCK / 64];
    if (gm_stopped(sc)) return;
    const long long stride = (long long)gridDim.x * BLOCK;
    double ss = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        double wi = w[i];
        int k0 = 0;
        for (; k0 + M <= c; k0 += M) {
            double v[M];
#pragma unroll
            for (int m = 0; m < M; ++m) v[m] = V[(long long)(k0 + m) * n + i];
#pragma unroll
            for (int m = 0; m < M; ++m) wi -= h[k0 + m] * v[m];
        }
        for (; k0 < c; ++k0) wi -= h[k0] * V[(long long)k0 * n + i];
        w[i] = wi;
        ss += wi * wi;
    }
    if (partN) {
        ss = gm_block_sum(ss, sh);
        if (threadIdx.x == 0) partN[blockIdx.x] = ss;
    }
}

// partN[block] = sum r^2 (the residual at the start of a cycle)
__global__ void __launch_bounds__(BLOCK) k_gm_sumsq(long long n, const double *__restrict__ r, double *__restrict__ partN,
                                                    const double *__restrict__ sc, int first)
{
    __shared__ double sh[BLOCK / 64];
    if (!first && gm_stopped(sc)) return;
    double ss = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) ss += r[i] * r[i];
    ss = gm_block_sum(ss, sh);
    if (threadIdx.x == 0) partN[blockIdx.x] = ss;
}

// dst = src / sc[which] (src and dst may be one vector)
__global__ void k_gm_scale(long long n, const double *src, double *dst, const double *__restrict__ sc, int which)
{
    if (gm_stopped(sc)) return;
    const double s = 1.0 / sc[which];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = s * src[i];
}

// t = sum_{k < K} y[k] V[k n + i] in the order of k, K = sc[GS_K]
template <int M>
__global__ void __launch_bounds__(BLOCK) k_gm_combine(long long n, const double *__restrict__ V, const double *__restrict__ y,
                                                      double *__restrict__ t, const double *__restrict__ sc)
{
    if (sc[GS_DONE] != 0.0) return;
    const int c = (int)sc[GS_K];
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        double ti = 0.0;
        int k0 = 0;
        for (; k0 + M <= c; k0 += M) {
            double v[M];
#pragma unroll
            for (int m = 0; m < M; ++m) v[m] = V[(long long)(k0 + m) * n + i];
#pragma unroll
            for (int m = 0; m < M; ++m) ti += y[k0 + m] * v[m];
        }
        for (; k0 < c; ++k0) ti += y[k0] * V[(long long)k0 * n + i];
        t[i] = ti;
    }
}

// x += z
__global__ void k_gm_axpy(long long n, const double *__restrict__ z, double *__restrict__ x, const double *__restrict__ sc)
{
    if (sc[GS_DONE] != 0.0) return;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) x[i] += z[i];
}

// one block: the partials added up in block order, then the scalars of the step `op`
//   GF_START    partN: r . r of the start residual -> beta, g_0; every scalar at its start value; stop = tol beta
//   GF_RESTART  partN: r . r of the residual formed again -> beta replaces g_0; beta <= stop: converged
//   GF_H1/_H2   part: the c columns' partials of a Gram-Schmidt pass -> hp (what k_gm_update takes off) and h = hp / h += hp
//   GF_ROT      partN: w . w -> h_{j+1,j}; the stored rotations applied to the new column, the new rotation, g, the stop
//   GF_NORM     partN: w . w -> sc[GS_HNEXT] only (igx_solver_gmres_orth_d)
//   GF_Y        the back substitution R y = g over the sc[GS_J] columns of the cycle -> y, sc[GS_K]
//   GF_CLOSE    after the update of x: the final one (GS_LAST) sets GS_DONE; else, if `more`, a restart follows
__global__ void __launch_bounds__(BLOCK) k_gm_fin(const double *part, int nb, int c, const double *partN, int nbN, Small a, int op,
                                                  double tol, int more)
{
    __shared__ double sh[BLOCK / 64];
    double *sc = a.sc;
    if (op == GF_H1 || op == GF_H2) {
        if (gm_stopped(sc)) return;
        for (int k = threadIdx.x; k < c; k += BLOCK) {
            double s = 0.0;
            for (int b = 0; b < nb; ++b) s += part[(long long)b * c + k];
            a.hp[k] = s;
            a.h[k] = op == GF_H1 ? s : a.h[k] + s;
        }
        return;
    }
    double nn = 0.0;
    if (op == GF_START || op == GF_RESTART || op == GF_ROT || op == GF_NORM) {
        for (int k = threadIdx.x; k < nbN; k += BLOCK) nn += partN[k];
        nn = gm_block_sum(nn, sh);
    }
    if (threadIdx.x != 0) return;
    if (op == GF_NORM) { sc[GS_HNEXT] = sqrt(nn); return; }
    if (op == GF_START) {
        for (int k = 0; k < GS_N; ++k) sc[k] = 0.0;
        if (!gm_finite(nn)) { sc[GS_DONE] = 1.0; sc[GS_REASON] = IGX_BREAKDOWN_NONFINITE; return; }
        const double beta = sqrt(nn);
        sc[GS_BETA] = a.g[0] = beta;
        sc[GS_STOP] = tol * beta;
        if (beta == 0.0) { sc[GS_DONE] = 1.0; sc[GS_CONV] = 1.0; }          // (the start vector solves the system)
        return;
    }
    if (sc[GS_DONE] != 0.0) return;
    if (op == GF_CLOSE) {
        if (sc[GS_LAST] != 0.0) sc[GS_DONE] = 1.0;
        else if (more) sc[GS_RESTARTS] += 1.0;
        return;
    }
    if (op == GF_Y) {
        const int K = (int)sc[GS_J];
        for (int i = K - 1; i >= 0; --i) {
            double t = a.g[i];
            for (int k = i + 1; k < K; ++k) t -= a.R[i + k * a.ld] * a.y[k];
            a.y[i] = t / a.R[i + i * a.ld];
        }
        bool ok = true;
        for (int i = 0; i < K; ++i) ok = ok && gm_finite(a.y[i]);
        if (!ok) { sc[GS_DONE] = 1.0; sc[GS_CONV] = 0.0; sc[GS_REASON] = IGX_BREAKDOWN_NONFINITE; return; }
        sc[GS_K] = (double)K;
        return;
    }
    if (sc[GS_LAST] != 0.0) return;
    if (op == GF_RESTART) {
        if (!gm_finite(nn)) { sc[GS_DONE] = 1.0; sc[GS_REASON] = IGX_BREAKDOWN_NONFINITE; return; }
        const double beta = sqrt(nn);
        sc[GS_BETA] = a.g[0] = beta;
        sc[GS_J] = 0.0;
        if (beta <= sc[GS_STOP]) { sc[GS_DONE] = 1.0; sc[GS_CONV] = 1.0; }
        return;
    }
    // GF_ROT
    const int j = (int)sc[GS_J];
    const double hn = sqrt(nn);
    bool ok = gm_finite(nn);
    for (int i = 0; i <= j; ++i) ok = ok && gm_finite(a.h[i]);
    if (!ok) { sc[GS_DONE] = 1.0; sc[GS_REASON] = IGX_BREAKDOWN_NONFINITE; return; }
    for (int i = 0; i < j; ++i) {
        const double t = a.cs[i] * a.h[i] + a.sn[i] * a.h[i + 1];
        a.h[i + 1] = a.cs[i] * a.h[i + 1] - a.sn[i] * a.h[i];
        a.h[i] = t;
    }
    const double rr = sqrt(a.h[j] * a.h[j] + hn * hn);
    if (rr == 0.0) { sc[GS_LAST] = 1.0; return; }   // (K z_j = 0: the matrix is singular on this space; the columns before j stand)
    const double cs = a.h[j] / rr, sn = hn / rr;
    const double gn = -sn * a.g[j], gj = cs * a.g[j];
    if (!gm_finite(gn) || !gm_finite(gj) || !gm_finite(rr)) { sc[GS_DONE] = 1.0; sc[GS_REASON] = IGX_BREAKDOWN_NONFINITE; return; }
    a.cs[j] = cs; a.sn[j] = sn;
    a.h[j] = rr;
    for (int i = 0; i <= j; ++i) a.R[i + j * a.ld] = a.h[i];
    a.g[j] = gj; a.g[j + 1] = gn;
    sc[GS_HNEXT] = hn;
    sc[GS_J] = (double)(j + 1);
    sc[GS_IT] += 1.0;
    // (h_{j+1,j} = 0, the lucky breakdown: the Krylov space holds the solution)
    if (fabs(gn) <= sc[GS_STOP] || hn == 0.0) { sc[GS_LAST] = 1.0; sc[GS_CONV] = 1.0; }
}

unsigned dot_blocks(long long n, int restart) { return std::min<unsigned>(vec_blocks(n), (unsigned)(GM_DOT_PART / (restart + 1))); }

// CGS2 of w against the first c columns of V, in place: the kernels of an Arnoldi step in their order, up to the partials of
// w . w (in s->d_part + GM_DOT_PART, vec_blocks(n) of them)
int orthogonalise(hipStream_t st, igx_solver *s, const Small &a, const double *V, int c, double *w)
{
    const long long n = s->n;
    const unsigned nbv = vec_blocks(n), nbd = dot_blocks(n, s->gm.restart);
    double *pD = s->d_part, *pN = s->d_part + GM_DOT_PART;
    for (int pass = 0; pass < 2; ++pass) {
        k_gm_dots<MB><<<nbd, BLOCK, 0, st>>>(n, V, c, w, pD, a.sc);
        k_gm_fin<<<1, BLOCK, 0, st>>>(pD, (int)nbd, c, nullptr, 0, a, pass == 0 ? GF_H1 : GF_H2, 0.0, 0);
        k_gm_update<MB><<<nbv, BLOCK, 0, st>>>(n, V, c, a.hp, w, pass == 1 ? pN : nullptr, a.sc);
    }
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

int read_small(hipStream_t st, const Small &a, double *h)
{
    IGX_HIP(hipMemcpyAsync(h, a.sc, GS_N * sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int inspection_args(igx_solver *s, const void *p1, const void *p2, int ncols, const char *what)
{
    if (!s || !p1 || !p2) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    if (!s->saddle) { set_error("%s: not a saddle-point solver (igx_solver_create_saddle)", what); return IGX_ERR_UNSUPPORTED; }
    if (s->gm.restart < 1) { set_error("%s: select GMRES first (igx_solver_set_gmres)", what); return IGX_ERR_ARG; }
    if (ncols < 1 || ncols > s->gm.restart + 1) {
        set_error("%s: %d columns, the solver holds 1 to restart + 1 = %d", what, ncols, s->gm.restart + 1);
        return IGX_ERR_ARG;
    }
    return IGX_OK;
}

} // namespace

namespace igx {

int solve_gmres(hipStream_t st, igx_solver *s, const double *rhs, double tol, int maxiter, int check_every, int timed, igx_solve_info &inf)
{
    SaddleState &S = s->sad;
    GmresState &G = s->gm;
    const long long n = s->n;
    const int m = G.restart;
    const Small a = small_of(G.d_small, G.cap);
    const unsigned nbv = vec_blocks(n);
    double *pN = s->d_part + GM_DOT_PART;
    double *V = G.d_V, *z = S.d_mvec + n, *t = S.d_mvec + 2 * n;
    hipEvent_t *E = s->ev;
    G.orth_ms = G.combine_ms = 0.0f;
    G.orth_count = G.combine_count = 0;
    G.restarts = 0;
    double h[GS_N] = {};
    int total = 0;
    // G.project_ops: every product and every preconditioned vector loses its pressure mean, so that the iteration runs on Q K Q and
    // Q P in the space of mean-free pressures (the partials of the sums are consumed before the next kernel writes d_part)
    auto project = [&](double *v) { return G.project_ops ? saddle_project_vector(st, s, v) : (int)IGX_OK; };
    for (int cycle = 0;; ++cycle) {
        // the cycle's start: v_0 = r / ||r||, r = rhs - K x (the first cycle: as the caller formed it, in s->r)
        const double *r = s->r;
        if (cycle > 0) {
            if (int rc = saddle_spmv(st, s, s->x, rhs, -1.0, V, nullptr, nullptr)) return rc;
            if (int rc = project(V)) return rc;
            r = V;
        }
        k_gm_sumsq<<<nbv, BLOCK, 0, st>>>(n, r, pN, a.sc, cycle == 0);
        k_gm_fin<<<1, BLOCK, 0, st>>>(nullptr, 0, 0, pN, (int)nbv, a, cycle == 0 ? GF_START : GF_RESTART, tol, 0);
        k_gm_scale<<<nbv, BLOCK, 0, st>>>(n, r, V, a.sc, GS_BETA);
        IGX_HIP(hipGetLastError());
        if (int rc = read_small(st, a, h)) return rc;
        for (int j = 0; j < m && total < maxiter && h[GS_DONE] == 0.0 && h[GS_LAST] == 0.0; ++j) {
            ++total;
            double *vj = V + (long long)j * n, *w = vj + n;
            if (timed) IGX_HIP(hipEventRecord(E[0], st));
            if (int rc = saddle_apply_precond(st, s, vj, z)) return rc;
            if (int rc = project(z)) return rc;
            if (timed) IGX_HIP(hipEventRecord(E[1], st));
            if (int rc = saddle_spmv(st, s, z, nullptr, 1.0, w, nullptr, nullptr)) return rc;
            if (int rc = project(w)) return rc;
            if (timed) IGX_HIP(hipEventRecord(E[2], st));
            if (int rc = orthogonalise(st, s, a, V, j + 1, w)) return rc;
            k_gm_fin<<<1, BLOCK, 0, st>>>(nullptr, 0, j + 1, pN, (int)nbv, a, GF_ROT, tol, 0);
            k_gm_scale<<<nbv, BLOCK, 0, st>>>(n, w, w, a.sc, GS_HNEXT);
            IGX_HIP(hipGetLastError());
            if (timed) IGX_HIP(hipEventRecord(E[3], st));
            if (timed || total % check_every == 0 || total == maxiter) {
                if (int rc = read_small(st, a, h)) return rc;
                if (timed) {
                    float ms[3] = {};
                    for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ms[k], E[k], E[k + 1]);
                    inf.precond_ms += ms[0]; inf.spmv_ms += ms[1]; inf.vector_ms += ms[2];
                    G.orth_ms += ms[2]; ++G.orth_count;
                }
            }
        }
        // the cycle's end (its m steps done, the stop met, or maxiter reached): x += P (V y)
        // (events 2 and 3 again: the steps are done with them, and 5 is the begin of the whole solve)
        if (timed) IGX_HIP(hipEventRecord(E[2], st));
        k_gm_fin<<<1, BLOCK, 0, st>>>(nullptr, 0, 0, nullptr, 0, a, GF_Y, tol, 0);
        k_gm_combine<MB><<<nbv, BLOCK, 0, st>>>(n, V, a.y, t, a.sc);
        IGX_HIP(hipGetLastError());
        if (int rc = saddle_apply_precond(st, s, t, z)) return rc;
        if (int rc = project(z)) return rc;
        k_gm_axpy<<<nbv, BLOCK, 0, st>>>(n, z, s->x, a.sc);
        k_gm_fin<<<1, BLOCK, 0, st>>>(nullptr, 0, 0, nullptr, 0, a, GF_CLOSE, tol, total < maxiter ? 1 : 0);
        IGX_HIP(hipGetLastError());
        if (timed) IGX_HIP(hipEventRecord(E[3], st));
        if (int rc = read_small(st, a, h)) return rc;
        if (timed) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, E[2], E[3]);
            inf.vector_ms += ms;
            G.combine_ms += ms; ++G.combine_count;
        }
        if (h[GS_DONE] != 0.0 || total >= maxiter) break;
    }
    inf.iterations = (int)h[GS_IT];
    inf.converged = h[GS_CONV] != 0.0 ? 1 : 0;
    S.breakdown = (int)h[GS_REASON];
    G.restarts = (int)h[GS_RESTARTS];
    return IGX_OK;
}

} // namespace igx

extern "C" {

int igx_solver_set_gmres(igx_solver *s, int restart, int triangular)
{
    const char *what = "igx_solver_set_gmres";
    if (!s) { set_error("%s: null solver", what); return IGX_ERR_ARG; }
    if (!s->saddle) {
        set_error("%s: GMRES serves saddle-point solvers (igx_solver_create_saddle) only", what);
        return IGX_ERR_UNSUPPORTED;
    }
    if (restart < 0 || restart > GM_MAX_RESTART) { set_error("%s: restart must be 0 (MINRES) or 1 to %d, not %d", what, GM_MAX_RESTART, restart); return IGX_ERR_ARG; }
    if (restart == 0 && triangular) {
        set_error("%s: the triangular preconditioner is not symmetric: MINRES (restart = 0) cannot take it", what);
        return IGX_ERR_ARG;
    }
    GmresState &G = s->gm;
    if (restart > G.cap) {
        IGX_HIP(hipSetDevice(s->ctx->device));
        IGX_HIP(hipStreamSynchronize(s->ctx->stream));
        double *V = nullptr, *sm = nullptr;
        const size_t nv = (size_t)(restart + 1) * (size_t)s->n;
        if (hipMalloc((void **)&V, nv * sizeof(double)) != hipSuccess || hipMalloc((void **)&sm, small_len(restart) * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(V);
            set_error("%s: out of device memory (%.3f GB for %d basis vectors)", what, 8.0 * nv / 1e9, restart + 1);
            return IGX_ERR_NOMEM;
        }
        hipError_t e = hipMemsetAsync(sm, 0, small_len(restart) * sizeof(double), s->ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);
        if (e != hipSuccess) { (void)hipFree(V); (void)hipFree(sm); set_error("%s: %s", what, hipGetErrorString(e)); return IGX_ERR_HIP; }
        (void)hipFree(G.d_V); (void)hipFree(G.d_small);
        G.d_V = V; G.d_small = sm; G.cap = restart;
    }
    G.restart = restart;
    G.triangular = triangular ? 1 : 0;
    return IGX_OK;
}

int igx_solver_gmres_orth_d(igx_solver *s, const double *d_V, int ncols, double *d_w, double *h_out, double *norm_out)
{
    const char *what = "igx_solver_gmres_orth_d";
    if (int rc = inspection_args(s, d_V, d_w, ncols, what)) return rc;
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const Small a = small_of(s->gm.d_small, s->gm.cap);
    IGX_HIP(hipMemsetAsync(a.sc, 0, GS_N * sizeof(double), st));
    IGX_HIP(hipEventRecord(s->ev[0], st));
    if (int rc = orthogonalise(st, s, a, d_V, ncols, d_w)) return rc;
    k_gm_fin<<<1, BLOCK, 0, st>>>(nullptr, 0, ncols, s->d_part + GM_DOT_PART, (int)vec_blocks(s->n), a, GF_NORM, 0.0, 0);
    IGX_HIP(hipGetLastError());
    if (int rc = close_call(st, s->ev[0], s->ev[1], what, s->gm.orth_ms)) return rc;
    s->gm.orth_count = 1;
    if (h_out) IGX_HIP(hipMemcpyAsync(h_out, a.h, (size_t)ncols * sizeof(double), hipMemcpyDeviceToHost, st));
    if (norm_out) IGX_HIP(hipMemcpyAsync(norm_out, a.sc + GS_HNEXT, sizeof(double), hipMemcpyDeviceToHost, st));
    IGX_HIP(hipStreamSynchronize(st));
    return IGX_OK;
}

int igx_solver_gmres_combine_d(igx_solver *s, const double *d_V, int ncols, const double *y, double *d_t)
{
    const char *what = "igx_solver_gmres_combine_d";
    if (int rc = inspection_args(s, d_V, d_t, ncols, what)) return rc;
    if (!y) { set_error("%s: null argument", what); return IGX_ERR_ARG; }
    IGX_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const Small a = small_of(s->gm.d_small, s->gm.cap);
    double sc[GS_N] = {};
    sc[GS_K] = (double)ncols;
    IGX_HIP(hipMemcpyAsync(a.sc, sc, sizeof(sc), hipMemcpyHostToDevice, st));
    IGX_HIP(hipMemcpyAsync(a.y, y, (size_t)ncols * sizeof(double), hipMemcpyHostToDevice, st));
    IGX_HIP(hipEventRecord(s->ev[0], st));
    k_gm_combine<MB><<<vec_blocks(s->n), BLOCK, 0, st>>>(s->n, d_V, a.y, d_t, a.sc);
    IGX_HIP(hipGetLastError());
    if (int rc = close_call(st, s->ev[0], s->ev[1], what, s->gm.combine_ms)) return rc;
    s->gm.combine_count = 1;
    return IGX_OK;
}

int igx_solver_gmres_timing(const igx_solver *s, float *orth_ms, float *combine_ms)
{
    if (!s || !s->saddle) { set_error("igx_solver_gmres_timing: not a saddle-point solver (igx_solver_create_saddle)"); return IGX_ERR_ARG; }
    if (orth_ms) *orth_ms = s->gm.orth_count ? s->gm.orth_ms / (float)s->gm.orth_count : 0.0f;
    if (combine_ms) *combine_ms = s->gm.combine_count ? s->gm.combine_ms / (float)s->gm.combine_count : 0.0f;
    return IGX_OK;
}

int igx_solver_gmres_restarts(const igx_solver *s) { return s && s->saddle ? s->gm.restarts : 0; }

} // extern "C"
