// Integrals over a patch from arrays on the resident Gauss points: sum W f_k (integrate) and the error sums
//     sum W (u_h - g)^2,   sum W |grad u_h - grad g|^2
// of a spline u_h of the patch's own space given by a DEVICE dof vector, total and per element.
//
// k_err12 is k_spline12 (kern_spline.hip) with the stores replaced: where that kernel writes value and gradient of a point, this
// one forms the differences to the exact arrays, squares, weighs with W = gw |det J| and sums along its grid line, element by
// element.  HBM sees the dofs, W and the exact arrays once, and one double per line and span.
//
// The summation order is fixed, whatever the launch geometry: inside a span of the last axis ascending Gauss index from 0.0
// (k_err12 / k_wsum: one lane per span reads the staged per-point terms), inside an element ascending (g0, g_mid) over its lines
// (k_quad_elems: one thread per element), over the elements a strided per-thread sum and a tree (k_quad_total: ONE block).  No
// atomics: two calls with the same inputs give the same bits.
#include "igx_internal.h"
#include "geo_device.h"
#include <algorithm>

namespace igx {

constexpr int Q_MAXWAVES = 4;
constexpr int Q_BLOCK = 256;
constexpr int Q_MAXF = 4;

struct QuadIn { const double *p[Q_MAXF]; };

// part[k][L][s] = sum_{j < q} stage[k][s q + j], ascending j from 0.0; lane s (+ 64 ..) owns span s.  The caller has made the
// wave's stores to `stage` visible.
__device__ __forceinline__ void span_sums(const double *stage, int nk, int Gl, int q, int Sl, int lane, double *part, long long kstride, long long L)
{
    for (int s = lane; s < Sl; s += 64)
        for (int k = 0; k < nk; ++k) {
            const double *t = stage + (size_t)k * Gl + (size_t)s * q;
            double acc = 0.0;
            for (int j = 0; j < q; ++j) acc += t[j];
            part[(size_t)k * kstride + L * Sl + s] = acc;
        }
}

__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The walk of k_spline12: a WAVE owns `lpw` consecutive lines; per line the mid-axis contraction goes into wave-private LDS lines
// of N_last doubles, the last-axis contraction is done per point.  Behind those lines the wave keeps 1 + GRAD lines of G_last
// doubles: the per-point terms W d0^2 and W sum_r dr^2, which lane s then sums over the q points of span s -- an element may
// straddle two passes of the point loop (q does not divide 64 in general), so the points cannot be summed where they are made.
//   ex.p[0]: exact values, ex.p[1 .. DIM]: exact physical gradient in jet order, each [npts_loc] or null (= 0)
//   part: [1 + GRAD][nlines][S_last]
template <int DIM, bool GRAD>
__global__ void __launch_bounds__(Q_MAXWAVES * 64) k_err12(const double *__restrict__ t0, const double *__restrict__ t1, const double *__restrict__ W,
                                                            const QuadIn ex, double *__restrict__ part,
                                                            const AxisDev am, const AxisDev al, const GeoView gv, const int nurbs,
                                                            const int g0_lo, const int gm_lo, const int Gm, const long long nlines, const int lpw)
{
    extern __shared__ double q_lds[];
    constexpr int NL = GRAD ? DIM : 1, NK = GRAD ? 2 : 1;
    const int Nl = al.N, Gl = al.G, Pl = al.P, ql = al.q, Sl = al.n, Pm = am.P, Nm = am.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    double *buf = q_lds + (size_t)wave * ((size_t)NL * Nl + (size_t)NK * Gl);
    double *stage = buf + (size_t)NL * Nl;
    const long long unit = (long long)blockIdx.x * nwaves + wave;
    const long long L_lo = unit * lpw, L_hi = min(L_lo + lpw, nlines);
    for (long long L = L_lo; L < L_hi; ++L) {
        const long long plane = L / Gm;
        const int gm = gm_lo + (int)(L - plane * Gm);
        {
            const double *Vm = am.V + (size_t)gm * Pm * 2;
            const long long row = (plane * Nm + am.fa[gm / am.q]) * Nl;
            for (int i = lane; i < Nl; i += 64) {
                double v = 0.0, dm = 0.0, d0 = 0.0;
                for (int l = 0; l < Pm; ++l) {
                    const double x = t0[row + (long long)l * Nl + i];
                    v = fma(Vm[2 * l], x, v);
                    if (GRAD) dm = fma(Vm[2 * l + 1], x, dm);
                    if (GRAD && DIM == 3) d0 = fma(Vm[2 * l], t1[row + (long long)l * Nl + i], d0);
                }
                buf[i] = v;
                if (GRAD) buf[Nl + i] = dm;
                if (GRAD && DIM == 3) buf[2 * Nl + i] = d0;
            }
        }
        wave_sync_lds();
        for (int g = lane; g < Gl; g += 64) {
            // the point's weight and exact values first: their loads are in flight during the contraction and the geometry
            const long long idx = L * Gl + g;
            const double w = W[idx];
            double e[1 + DIM];
            e[0] = ex.p[0] ? ex.p[0][idx] : 0.0;
#pragma unroll
            for (int r = 1; r <= DIM; ++r) e[r] = GRAD && ex.p[1] ? ex.p[r][idx] : 0.0;
            const double *Vl = al.V + (size_t)g * Pl * 2;
            const double *b = buf + al.fa[g / ql];
            double v = 0.0, gp[3] = {0.0, 0.0, 0.0};          // parametric gradient in jet order: last, mid, axis 0
            for (int l = 0; l < Pl; ++l) {
                const double n = Vl[2 * l], x = b[l];
                v = fma(n, x, v);
                if (GRAD) {
                    gp[0] = fma(Vl[2 * l + 1], x, gp[0]);
                    gp[1] = fma(n, b[Nl + l], gp[1]);
                    if (DIM == 3) gp[2] = fma(n, b[2 * Nl + l], gp[2]);
                }
            }
            const double d0 = v - e[0];
            stage[g] = w * (d0 * d0);
            if (GRAD) {
                int gi[3];
                if (DIM == 3) { gi[0] = g0_lo + (int)plane; gi[1] = gm; gi[2] = g; }
                else { gi[0] = gm; gi[1] = g; gi[2] = 0; }
                double pg[3];
                physical_gradient<DIM>(gv, nurbs != 0, gi, gp, pg);
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < DIM; ++r) {
                    const double dr = pg[r] - e[1 + r];
                    s += dr * dr;
                }
                stage[Gl + g] = w * s;
            }
        }
        wave_sync_lds();
        span_sums(stage, NK, Gl, ql, Sl, lane, part, nlines * Sl, L);
        // the next line overwrites buf and stage
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// Element residual sums  sum W (f + Lap u_h)^2  and  sum W  (DESIGN.md section 38): the walk of k_err12 with the parametric
// gradient AND Hessian of u_h contracted.  The wave's LDS lines hold the mid-axis contractions of every (axis-0 order, mid order)
// of total order <= 2 -- 2D: mid orders 0, 1, 2 of the dofs; 3D: (0,0) (0,1) (0,2) of t0, (1,0) (1,1) of t1, (2,0) of t2 -- and the
// point loop contracts the last axis with orders 0, 1, 2.  The second-derivative tables are [P][G] (d2m, d2l; the geometry's in g2).
//   Lap u_h = sum_cd K_cd D_c D_d u^ + sum_c b_c D_c u^   (laplace_coefficients, geo_device.h)
//   part: [2][nlines][S_last]: W (f + Lap u_h)^2, W
template <int DIM>
__global__ void __launch_bounds__(Q_MAXWAVES * 64) k_res12(const double *__restrict__ t0, const double *__restrict__ t1, const double *__restrict__ t2,
                                                            const double *__restrict__ W, const double *__restrict__ f, double *__restrict__ part,
                                                            const AxisDev am, const AxisDev al, const double *__restrict__ d2m,
                                                            const double *__restrict__ d2l, const GeoView gv, const GeoView2 g2, const int nurbs,
                                                            const int g0_lo, const int gm_lo, const int Gm, const long long nlines, const int lpw)
{
    extern __shared__ double q_lds[];
    constexpr int NL = DIM == 3 ? 6 : 3;
    const int Nl = al.N, Gl = al.G, Pl = al.P, ql = al.q, Sl = al.n, Pm = am.P, Nm = am.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    double *buf = q_lds + (size_t)wave * ((size_t)NL * Nl + (size_t)2 * Gl);
    double *stage = buf + (size_t)NL * Nl;
    const long long unit = (long long)blockIdx.x * nwaves + wave;
    const long long L_lo = unit * lpw, L_hi = min(L_lo + lpw, nlines);
    for (long long L = L_lo; L < L_hi; ++L) {
        const long long plane = L / Gm;
        const int gm = gm_lo + (int)(L - plane * Gm);
        {
            const double *Vm = am.V + (size_t)gm * Pm * 2;
            const double *Dm = d2m + gm;
            const long long row = (plane * Nm + am.fa[gm / am.q]) * Nl;
            for (int i = lane; i < Nl; i += 64) {
                double v = 0.0, dm = 0.0, ddm = 0.0, v1 = 0.0, dm1 = 0.0, v2 = 0.0;
                for (int l = 0; l < Pm; ++l) {
                    const double n = Vm[2 * l], d = Vm[2 * l + 1], dd = Dm[(size_t)l * am.G];
                    const double x = t0[row + (long long)l * Nl + i];
                    v = fma(n, x, v);
                    dm = fma(d, x, dm);
                    ddm = fma(dd, x, ddm);
                    if (DIM == 3) {
                        const double x1 = t1[row + (long long)l * Nl + i];
                        v1 = fma(n, x1, v1);
                        dm1 = fma(d, x1, dm1);
                        v2 = fma(n, t2[row + (long long)l * Nl + i], v2);
                    }
                }
                buf[i] = v;
                buf[Nl + i] = dm;
                buf[2 * Nl + i] = ddm;
                if (DIM == 3) {
                    buf[3 * Nl + i] = v1;
                    buf[4 * Nl + i] = dm1;
                    buf[5 * Nl + i] = v2;
                }
            }
        }
        wave_sync_lds();
        for (int g = lane; g < Gl; g += 64) {
            // the point's weight and right-hand side first: their loads are in flight during the contraction and the geometry
            const long long idx = L * Gl + g;
            const double w = W[idx];
            const double fv = f ? f[idx] : 0.0;
            const double *Vl = al.V + (size_t)g * Pl * 2;
            const double *Dl = d2l + g;
            const double *b = buf + al.fa[g / ql];
            // parametric gradient and Hessian in jet order (0: last axis, 1: mid, 2: axis 0), the Hessian packed 00 01 [02] 11 [12 22]
            double gp[3] = {0.0, 0.0, 0.0}, H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int l = 0; l < Pl; ++l) {
                const double n = Vl[2 * l], d = Vl[2 * l + 1], dd = Dl[(size_t)l * Gl];
                const double x = b[l], xm = b[Nl + l], xmm = b[2 * Nl + l];
                gp[0] = fma(d, x, gp[0]);
                gp[1] = fma(n, xm, gp[1]);
                H[0] = fma(dd, x, H[0]);
                H[1] = fma(d, xm, H[1]);
                if (DIM == 2) H[2] = fma(n, xmm, H[2]);
                else {
                    const double x0 = b[3 * Nl + l];
                    gp[2] = fma(n, x0, gp[2]);
                    H[2] = fma(d, x0, H[2]);
                    H[3] = fma(n, xmm, H[3]);
                    H[4] = fma(n, b[4 * Nl + l], H[4]);
                    H[5] = fma(n, b[5 * Nl + l], H[5]);
                }
            }
            int gi[3];
            if (DIM == 3) { gi[0] = g0_lo + (int)plane; gi[1] = gm; gi[2] = g; }
            else { gi[0] = gm; gi[1] = g; gi[2] = 0; }
            double K[6], bc[3];
            laplace_coefficients<DIM>(gv, g2, nurbs != 0, gi, K, bc);
            double lap = 0.0;
#pragma unroll
            for (int c = 0; c < DIM; ++c)
#pragma unroll
                for (int d = c; d < DIM; ++d) {
                    const int t = sym_index<DIM>(c, d);
                    lap = fma(c == d ? K[t] : 2.0 * K[t], H[t], lap);
                }
#pragma unroll
            for (int c = 0; c < DIM; ++c) lap = fma(bc[c], gp[c], lap);
            const double r = fv + lap;
            stage[g] = w * (r * r);
            stage[Gl + g] = w;
        }
        wave_sync_lds();
        span_sums(stage, 2, Gl, ql, Sl, lane, part, nlines * Sl, L);
        // the next line overwrites buf and stage
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// part[k][L][s] = sum over the q points of span s of line L of W f_k, k < nf: the accumulation stage of k_err12 alone
__global__ void __launch_bounds__(Q_MAXWAVES * 64) k_wsum(const double *__restrict__ W, const QuadIn f, const int nf, double *__restrict__ part,
                                                           const int Gl, const int ql, const int Sl, const long long nlines, const int lpw)
{
    extern __shared__ double q_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    double *stage = q_lds + (size_t)wave * nf * Gl;
    const long long unit = (long long)blockIdx.x * nwaves + wave;
    const long long L_lo = unit * lpw, L_hi = min(L_lo + lpw, nlines);
    for (long long L = L_lo; L < L_hi; ++L) {
        for (int g = lane; g < Gl; g += 64) {
            const long long idx = L * Gl + g;
            const double w = W[idx];
            for (int k = 0; k < nf; ++k) stage[(size_t)k * Gl + g] = w * f.p[k][idx];
        }
        wave_sync_lds();
        span_sums(stage, nf, Gl, ql, Sl, lane, part, nlines * Sl, L);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// elem[k][s0][sm][sl] = sum of the q0 qm partial lines of the element in ascending (g0, g_mid) order (2D: Sm = qm = Gm = 1, the
// lines are the Gauss points of axis 0).  One thread per element, consecutive threads consecutive sl.
__global__ void __launch_bounds__(Q_BLOCK) k_quad_elems(const double *__restrict__ part, double *__restrict__ elem, const int nk, const long long nelem,
                                                         const long long nlines, const int Sm, const int Sl, const int q0, const int qm, const int Gm)
{
    const long long idx = (long long)blockIdx.x * Q_BLOCK + threadIdx.x;
    if (idx >= nk * nelem) return;
    const long long k = idx / nelem, e = idx - k * nelem;
    const int sl = (int)(e % Sl);
    const long long t = e / Sl;
    const int sm = (int)(t % Sm);
    const long long s0 = t / Sm;
    const double *p = part + k * nlines * Sl + sl;
    double acc = 0.0;
    for (int a = 0; a < q0; ++a)
        for (int b = 0; b < qm; ++b)
            acc += p[((s0 * q0 + a) * Gm + ((long long)sm * qm + b)) * Sl];
    elem[idx] = acc;
}

__device__ __forceinline__ double quad_block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = Q_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    const double s = sh[0];
    __syncthreads();
    return s;
}

// one block: tot[k] = sum of elem[k][*], a strided per-thread sum and a tree (the shape of k_fin, solve.hip)
__global__ void __launch_bounds__(Q_BLOCK) k_quad_total(const double *__restrict__ elem, const int nk, const long long nelem, double *__restrict__ tot)
{
    __shared__ double sh[Q_BLOCK];
    for (int k = 0; k < nk; ++k) {
        double a = 0.0;
        for (long long i = threadIdx.x; i < nelem; i += Q_BLOCK) a += elem[k * nelem + i];
        a = quad_block_sum(a, sh);
        if (threadIdx.x == 0) tot[k] = a;
    }
}

// waves per block such that `per_wave` doubles of LDS each fit the 64 KB a block gets by default (0: not even one does)
static int quad_waves(size_t per_wave)
{
    for (int w = Q_MAXWAVES; w >= 1; w >>= 1)
        if ((size_t)w * per_wave * sizeof(double) <= 64 * 1024) return w;
    return 0;
}

struct QuadShape {
    int Sm, Sl, q0, qm, Gm;
    long long nlines, nelem;
    int lpw;
};

// whole, unboxed patches only (the caller has checked): the resident slab is the Gauss grid
static QuadShape quad_shape(const igx_patch *pt)
{
    const PatchDev &pd = pt->dev;
    QuadShape s{};
    if (pd.dim == 3) {
        s.Sm = pd.ax[1].n; s.Sl = pd.ax[2].n; s.q0 = pd.ax[0].q; s.qm = pd.ax[1].q; s.Gm = pd.ax[1].G;
        s.nlines = (long long)pd.G0_loc * s.Gm;
        s.nelem = (long long)pd.ax[0].n * s.Sm * s.Sl;
    } else {
        s.Sm = 1; s.Sl = pd.ax[1].n; s.q0 = pd.ax[0].q; s.qm = 1; s.Gm = 1;
        s.nlines = pd.G0_loc;
        s.nelem = (long long)pd.ax[0].n * s.Sl;
    }
    // enough waves for the chip before a wave takes more than one line (as k_spline12)
    s.lpw = (int)std::min<long long>(8, std::max<long long>(1, s.nlines / 16384));
    return s;
}

// doubles of the partial-line array, the element sums and the totals for nk quantities
size_t quad_workspace(const igx_patch *pt, int nk)
{
    const QuadShape s = quad_shape(pt);
    return (size_t)nk * ((size_t)s.nlines * s.Sl + (size_t)s.nelem) + Q_MAXF;
}

// partial lines -> element sums (d_elem, or the workspace) -> totals -> host
static int quad_finish(hipStream_t st, const QuadShape &s, int nk, double *d_ws, double *d_elem, double **d_tot)
{
    double *part = d_ws, *elem = d_elem ? d_elem : d_ws + (size_t)nk * s.nlines * s.Sl;
    *d_tot = d_ws + (size_t)nk * ((size_t)s.nlines * s.Sl + (size_t)s.nelem);
    const long long n = nk * s.nelem;
    k_quad_elems<<<dim3((unsigned)((n + Q_BLOCK - 1) / Q_BLOCK)), Q_BLOCK, 0, st>>>(part, elem, nk, s.nelem, s.nlines, s.Sm, s.Sl, s.q0, s.qm, s.Gm);
    IGX_HIP(hipGetLastError());
    k_quad_total<<<1, Q_BLOCK, 0, st>>>(elem, nk, s.nelem, *d_tot);
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

// d_f[0 .. nf): arrays over the resident slab; d_W the weight field; d_ws: quad_workspace(pt, nf) doubles; *d_tot: where the nf
// totals are (inside d_ws).  The caller has checked the patch (whole, not boxed) and 1 <= nf <= 4.
int launch_quad_sums(hipStream_t st, const igx_patch *pt, int nf, const double *const *d_f, const double *d_W, double *d_elem, double *d_ws,
                     double **d_tot, int *n_launches)
{
    const PatchDev &pd = pt->dev;
    const AxisDev &al = pd.dim == 3 ? pd.ax[2] : pd.ax[1];
    const QuadShape s = quad_shape(pt);
    const size_t per_wave = (size_t)nf * al.G;
    const int nw = quad_waves(per_wave);
    if (nw == 0) { set_error("igx_patch_quad_sums_d: %d Gauss points on the last axis do not fit the line buffers", al.G); return IGX_ERR_UNSUPPORTED; }
    QuadIn f{};
    for (int k = 0; k < nf; ++k) f.p[k] = d_f[k];
    const long long units = (s.nlines + s.lpw - 1) / s.lpw;
    k_wsum<<<dim3((unsigned)((units + nw - 1) / nw)), nw * 64, nw * per_wave * sizeof(double), st>>>(d_W, f, nf, d_ws, al.G, al.q, al.n, s.nlines, s.lpw);
    IGX_HIP(hipGetLastError());
    *n_launches = 3;
    return quad_finish(st, s, nf, d_ws, d_elem, d_tot);
}

// LDS doubles per wave of k_err12: the lines of k_spline12 and the staged per-point terms
static size_t err12_per_wave(int dim, bool grad, int Nlast, int Glast)
{
    return (size_t)(grad ? dim : 1) * Nlast + (size_t)(grad ? 2 : 1) * Glast;
}

// d_coeffs: the dofs; d_exact[0 .. dim]: exact arrays or null; d_sp_ws: spline_eval_workspace() doubles; d_ws: quad_workspace(pt,
// 1 + want_grad) doubles.  The caller has checked the patch (whole, not boxed, a spline geometry for the gradient).
int launch_error_sums(hipStream_t st, const igx_patch *pt, const double *d_coeffs, int want_grad, const double *const d_exact[4], const double *d_W,
                      double *d_elem, double *d_sp_ws, double *d_ws, double **d_tot, int *n_launches)
{
    const PatchDev &pd = pt->dev;
    const int dim = pd.dim;
    const AxisDev &am = dim == 3 ? pd.ax[1] : pd.ax[0], &al = dim == 3 ? pd.ax[2] : pd.ax[1];
    const bool grad = want_grad != 0;
    const QuadShape s = quad_shape(pt);
    const size_t per_wave = err12_per_wave(dim, grad, al.N, al.G);
    const int nw = quad_waves(per_wave);
    if (nw == 0) { set_error("igx_patch_error_sums_d: %d dofs and %d Gauss points on the last axis do not fit the line buffers", al.N, al.G); return IGX_ERR_UNSUPPORTED; }
    const double *t0 = nullptr, *t1 = nullptr;
    if (int rc = launch_spline_axis0(st, pt, d_coeffs, want_grad, d_sp_ws, &t0, &t1)) return rc;
    QuadIn ex{};
    ex.p[0] = d_exact ? d_exact[0] : nullptr;
    for (int r = 1; r <= dim; ++r) ex.p[r] = grad && d_exact ? d_exact[r] : nullptr;
    GeoView gv{};
    if (grad) gv = make_view(dim, pt->gax, pt->d_ctrl, pt->ncomp);
    const int nurbs = pt->geo_kind == IGX_GEO_NURBS ? 1 : 0;
    const int gm_lo = dim == 3 ? 0 : pd.g0_lo, Gm = dim == 3 ? am.G : pd.G0_loc;
    const long long units = (s.nlines + s.lpw - 1) / s.lpw;
    const dim3 grid((unsigned)((units + nw - 1) / nw));
    const size_t lds = nw * per_wave * sizeof(double);
#define ERR(D_, G_) k_err12<D_, G_><<<grid, nw * 64, lds, st>>>(t0, t1, d_W, ex, d_ws, am, al, gv, nurbs, pd.g0_lo, gm_lo, Gm, s.nlines, s.lpw)
    if (dim == 3) { if (grad) ERR(3, true); else ERR(3, false); }
    else { if (grad) ERR(2, true); else ERR(2, false); }
#undef ERR
    IGX_HIP(hipGetLastError());
    *n_launches = dim == 3 ? 4 : 3;
    return quad_finish(st, s, grad ? 2 : 1, d_ws, d_elem, d_tot);
}

// LDS doubles per wave of k_res12: 3 (2D) or 6 (3D) lines of N_last and the two staged per-point terms
static size_t res12_per_wave(int dim, int Nlast, int Glast)
{
    return (size_t)(dim == 3 ? 6 : 3) * Nlast + (size_t)2 * Glast;
}

// value, first and second axis-0 derivative planes (3D; 2D: k_res12 reads the dofs)
size_t residual_spline_workspace(const igx_patch *pt)
{
    const PatchDev &pd = pt->dev;
    return pd.dim == 3 ? (size_t)3 * pd.G0_loc * pd.ax[1].N * pd.ax[2].N : 0;
}

// The order-0, 1, 2 tables of every axis at its Gauss nodes, for the solution space and for the geometry space, made once per
// patch by the routine that fills the order-2 slots of igx_patch_set_basis_orders (launch_basis_tables); V, PI and the orders of
// the patch's own tables are not touched.
int residual_tables(hipStream_t st, igx_patch *pt)
{
    if (pt->tab2_ready) return IGX_OK;
    for (int k = 0; k < pt->dim; ++k) {
        const Axis &A = pt->ax[k];
        const GeoAxis &g = pt->gax[k];
        if (!pt->d_tab2[k]) IGX_HIP(hipMalloc((void **)&pt->d_tab2[k], std::max<size_t>(1, (size_t)3 * A.P * A.G) * sizeof(double)));
        if (!pt->d_gtab2[k]) IGX_HIP(hipMalloc((void **)&pt->d_gtab2[k], std::max<size_t>(1, (size_t)3 * g.P * A.G) * sizeof(double)));
        if (int rc = launch_basis_tables(st, A.d_kv, (int)A.kv.size(), A.p, A.d_nodes, (size_t)A.G, 2, pt->d_tab2[k], nullptr, nullptr, nullptr)) return rc;
        if (int rc = launch_basis_tables(st, g.d_kv, (int)g.kv.size(), g.p, A.d_nodes, (size_t)A.G, 2, pt->d_gtab2[k], nullptr, nullptr, nullptr)) return rc;
    }
    IGX_HIP(hipStreamSynchronize(st));
    pt->tab2_ready = true;
    return IGX_OK;
}

// d_coeffs: the dofs; d_f: the right-hand side over the resident slab or null; d_sp_ws: residual_spline_workspace() doubles; d_ws:
// quad_workspace(pt, 2) doubles.  The caller has checked the patch (whole, not boxed, a spline geometry) and made the tables.
int launch_residual_sums(hipStream_t st, const igx_patch *pt, const double *d_coeffs, const double *d_f, const double *d_W,
                         double *d_elem, double *d_sp_ws, double *d_ws, double **d_tot, int *n_launches)
{
    const PatchDev &pd = pt->dev;
    const int dim = pd.dim;
    const int km = dim == 3 ? 1 : 0, kl = dim == 3 ? 2 : 1;
    const AxisDev &am = pd.ax[km], &al = pd.ax[kl];
    const QuadShape s = quad_shape(pt);
    const size_t per_wave = res12_per_wave(dim, al.N, al.G);
    const int nw = quad_waves(per_wave);
    if (nw == 0) { set_error("igx_patch_residual_sums_d: %d dofs and %d Gauss points on the last axis do not fit the line buffers", al.N, al.G); return IGX_ERR_UNSUPPORTED; }
    auto d2 = [&](int k) { return pt->d_tab2[k] + (size_t)2 * pt->ax[k].P * pt->ax[k].G; };
    const double *t0 = d_coeffs, *t1 = nullptr, *t2 = nullptr;
    if (dim == 3) {
        if (int rc = launch_spline_axis0_d2(st, pt, d_coeffs, d2(0), d_sp_ws)) return rc;
        const size_t total = (size_t)pd.G0_loc * pd.ax[1].N * pd.ax[2].N;
        t0 = d_sp_ws; t1 = d_sp_ws + total; t2 = d_sp_ws + 2 * total;
    }
    const GeoView gv = make_view(dim, pt->gax, pt->d_ctrl, pt->ncomp);
    GeoView2 g2{};
    for (int k = 0; k < dim; ++k) { g2.D2[k] = pt->d_gtab2[k] + (size_t)2 * pt->gax[k].P * pt->ax[k].G; g2.G[k] = pt->ax[k].G; }
    const int nurbs = pt->geo_kind == IGX_GEO_NURBS ? 1 : 0;
    const int gm_lo = dim == 3 ? 0 : pd.g0_lo, Gm = dim == 3 ? am.G : pd.G0_loc;
    const long long units = (s.nlines + s.lpw - 1) / s.lpw;
    const dim3 grid((unsigned)((units + nw - 1) / nw));
    const size_t lds = nw * per_wave * sizeof(double);
#define RES(D_) k_res12<D_><<<grid, nw * 64, lds, st>>>(t0, t1, t2, d_W, d_f, d_ws, am, al, d2(km), d2(kl), gv, g2, nurbs, pd.g0_lo, gm_lo, Gm, s.nlines, s.lpw)
    if (dim == 3) RES(3); else RES(2);
#undef RES
    IGX_HIP(hipGetLastError());
    *n_launches = dim == 3 ? 4 : 3;
    return quad_finish(st, s, 2, d_ws, d_elem, d_tot);
}

} // namespace igx
