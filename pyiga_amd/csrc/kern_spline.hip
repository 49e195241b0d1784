// A spline of the patch's own space, given by a DEVICE dof vector, evaluated at the resident Gauss points: value and
// (optionally) physical gradient.  The input of iterate-dependent form coefficients (Newton's method: DESIGN.md section 19).
//
// It is the transpose of the load-vector contraction (kern_vector.hip): per axis
//     out[a][g][b] = sum_{l < P} V[g][l][deriv] * in[a][fa[g / q] + l][b]
// with the resident AxisDev tables.  Axis 0 is expanded first (3D): the arrays stay small -- [G0][N1][N2] -- until the last
// pass, and k_spline12 expands the mid and the last axis of one grid line in one go, the mirror of k_lv12: the intermediate
// [G0][G1][N2] lives in LDS, a line at a time, and HBM sees the dofs once and the 8 bytes per point and output array of the
// store stream.  Value and all parametric derivatives come out of one pass; J^-T is applied before the stores.
#include "igx_internal.h"
#include "geo_device.h"
#include <algorithm>

namespace igx {

// 3D, axis 0: t[d][g][j] = sum_l V0[g0_lo + g][l][d] * c[fa0 + l][j], j over the N1 * N2 dofs of a plane; d = 0 (value) and, with
// ND = 2, d = 1 (derivative along axis 0) from the same loads
template <int ND>
__global__ void __launch_bounds__(256) k_spline_axis0(const double *__restrict__ c, double *__restrict__ t, const AxisDev a0,
                                                      int g0_lo, int G0, long long B)
{
    const long long total = (long long)G0 * B;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int g = (int)(idx / B);
    const long long j = idx - (long long)g * B;
    const int gg = g0_lo + g, P = a0.P;
    const double *V = a0.V + (size_t)gg * P * 2;
    const double *src = c + (long long)a0.fa[gg / a0.q] * B + j;
    double r0 = 0.0, r1 = 0.0;
    for (int l = 0; l < P; ++l) {
        const double x = src[(long long)l * B];
        r0 = fma(V[2 * l], x, r0);
        if (ND == 2) r1 = fma(V[2 * l + 1], x, r1);
    }
    t[idx] = r0;
    if (ND == 2) t[total + idx] = r1;
}

// The same with the second derivative along axis 0 as a third array, for the residual sums (kern_quad.hip): d2 is the axis'
// second-derivative table [P][G0] (launch_basis_tables' plain output).  A sibling, so that k_spline_axis0 keeps its code.
__global__ void __launch_bounds__(256) k_spline_axis0_d2(const double *__restrict__ c, double *__restrict__ t, const AxisDev a0,
                                                         const double *__restrict__ d2, int g0_lo, int G0, long long B)
{
    const long long total = (long long)G0 * B;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int g = (int)(idx / B);
    const long long j = idx - (long long)g * B;
    const int gg = g0_lo + g, P = a0.P;
    const double *V = a0.V + (size_t)gg * P * 2;
    const double *src = c + (long long)a0.fa[gg / a0.q] * B + j;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int l = 0; l < P; ++l) {
        const double x = src[(long long)l * B];
        r0 = fma(V[2 * l], x, r0);
        r1 = fma(V[2 * l + 1], x, r1);
        r2 = fma(d2[(size_t)l * a0.G + gg], x, r2);
    }
    t[idx] = r0;
    t[total + idx] = r1;
    t[2 * total + idx] = r2;
}

// 3D: value, first and second axis-0 derivative planes of the dofs into d_ws (3 G0 N1 N2 doubles); 2D: nothing to do
int launch_spline_axis0_d2(hipStream_t st, const igx_patch *pt, const double *d_coeffs, const double *d_d2, double *d_ws)
{
    const PatchDev &pd = pt->dev;
    if (pd.dim != 3) return IGX_OK;
    const long long B = (long long)pd.ax[1].N * pd.ax[2].N, total = (long long)pd.G0_loc * B;
    k_spline_axis0_d2<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(d_coeffs, d_ws, pd.ax[0], d_d2, pd.g0_lo, pd.G0_loc, B);
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

struct SplineOut { double *o[4]; };

// Mid and last axis of a grid line.  A WAVE owns `lpw` consecutive lines (plane, Gauss index gm of the mid axis).  Per line:
// lane i (+ 64, + 128 ..) contracts the P rows fa_m + l of the plane with the mid axis' basis values (and derivatives) into
// wave-private LDS lines of N_last doubles -- value, d/d mid, and in 3D the same of the axis-0 derivative plane --; then lane g
// (+ 64 ..) sums its P active functions of the last axis from those lines and stores: consecutive lanes, consecutive doubles.
// No block barrier: a wave's LDS accesses complete in order.
//   t0: [planes][N_mid][N_last] value along axis 0 (2D: the dofs themselves, one plane); t1: derivative along axis 0 (3D, GRAD)
//   jet order of the outputs: o[0] value, o[1] d/dx (x = last grid axis), o[2] d/dy, o[3] d/dz -- physical when a geometry is given
constexpr int SP_MAXWAVES = 4;
template <int DIM, bool GRAD>
__global__ void __launch_bounds__(SP_MAXWAVES * 64) k_spline12(const double *__restrict__ t0, const double *__restrict__ t1, const SplineOut out,
                                                                const AxisDev am, const AxisDev al, const GeoView gv, const int nurbs,
                                                                const int g0_lo, const int gm_lo, const int Gm, const long long nlines, const int lpw)
{
    extern __shared__ double sp_lds[];
    constexpr int NL = GRAD ? DIM : 1;
    const int Nl = al.N, Gl = al.G, Pl = al.P, ql = al.q, Pm = am.P, Nm = am.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    double *buf = sp_lds + (size_t)wave * NL * Nl;
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
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int g = lane; g < Gl; g += 64) {
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
            const long long idx = L * Gl + g;
            out.o[0][idx] = v;
            if (GRAD) {
                int gi[3];
                if (DIM == 3) { gi[0] = g0_lo + (int)plane; gi[1] = gm; gi[2] = g; }
                else { gi[0] = gm; gi[1] = g; gi[2] = 0; }
                double pg[3];
                physical_gradient<DIM>(gv, nurbs != 0, gi, gp, pg);
#pragma unroll
                for (int r = 0; r < DIM; ++r) out.o[1 + r][idx] = pg[r];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// The inverse geometry Jacobian of one point, kept apart from its application so that a vector-valued spline evaluates and
// inverts it once for all its components.  The two halves together are the text of physical_gradient (geo_device.h), operation
// for operation: a component of k_vspline12 has the bits of k_spline12 on that component's dofs.
template <int DIM>
struct GradMap { double a[9]; double inv; };

template <int DIM>
__device__ __forceinline__ void gradient_map(const GeoView &gv, bool nurbs, const int gi[3], GradMap<DIM> &M)
{
    double Jm[MAX_COMP][3], ev[MAX_COMP];
    physical_jacobian<DIM>(gv, nurbs, gi, DIM, Jm, ev);
    if (DIM == 2) {
        M.inv = 1.0 / (Jm[0][0] * Jm[1][1] - Jm[0][1] * Jm[1][0]);
        M.a[0] = Jm[0][0]; M.a[1] = Jm[0][1]; M.a[2] = Jm[1][0]; M.a[3] = Jm[1][1];
    } else {
        const double t[9] = {Jm[0][0], Jm[0][1], Jm[0][2], Jm[1][0], Jm[1][1], Jm[1][2], Jm[2][0], Jm[2][1], Jm[2][2]};
        const double t3 = t[4] * t[8] - t[5] * t[7];
        const double t4 = t[3] * t[8] - t[5] * t[6];
        const double t5 = t[3] * t[7] - t[4] * t[6];
        const double inv = 1.0 / ((t[0] * t3 - t[1] * t4) + t[2] * t5);
        double *JI = M.a;
        JI[0] = inv * t3;
        JI[1] = inv * -(t[1] * t[8] - t[2] * t[7]);
        JI[2] = inv * (t[1] * t[5] - t[2] * t[4]);
        JI[3] = inv * -t4;
        JI[4] = inv * (t[0] * t[8] - t[2] * t[6]);
        JI[5] = inv * -(t[0] * t[5] - t[2] * t[3]);
        JI[6] = inv * t5;
        JI[7] = inv * -(t[0] * t[7] - t[1] * t[6]);
        JI[8] = inv * (t[0] * t[4] - t[1] * t[3]);
        M.inv = inv;
    }
}

template <int DIM>
__device__ __forceinline__ void apply_gradient_map(const GradMap<DIM> &M, const double gp[3], double pg[3])
{
    if (DIM == 2) {
        pg[0] = M.inv * (M.a[3] * gp[0] - M.a[2] * gp[1]);
        pg[1] = M.inv * (M.a[0] * gp[1] - M.a[1] * gp[0]);
    } else {
        // (JI[r] gp0 + JI[3 + r] gp1) + JI[6 + r] gp2 with the contractions spelled out as the compiler chooses them in
        // physical_gradient, where every JI has one use: of the two inner products the one whose JI carries the minus sign of its
        // cofactor (JI[3], JI[1], JI[5]) is rounded on its own, the other two are fused.  Left to the compiler, the shared JI of
        // this kernel fuse the other way round for r = 1 (tests/test_vspline_gpu.py compares the bits).
        const double *JI = M.a;
        pg[0] = fma(JI[6], gp[2], fma(JI[0], gp[0], JI[3] * gp[1]));
        pg[1] = fma(JI[7], gp[2], fma(JI[4], gp[1], JI[1] * gp[0]));
        pg[2] = fma(JI[8], gp[2], fma(JI[2], gp[0], JI[5] * gp[1]));
    }
}

// NC splines of the patch's space at once (the velocity of a saddle-point vector: component-major dofs): k_spline12 with the
// mid-axis contraction of every component in the wave's LDS lines -- component c owns the lines [c NL, (c + 1) NL) of the wave's
// buffer -- and ONE evaluation and inversion of the geometry Jacobian per point, applied to every component before the stores.
//   t0 / t1: as in k_spline12, component c at t0 + c * cstride (t1 likewise)
//   o[c]: value of component c; o[NC + c DIM + r]: its physical partial r in jet order (GRAD)
struct VSplineOut { double *o[12]; };

template <int DIM, int NC, bool GRAD>
__global__ void __launch_bounds__(SP_MAXWAVES * 64) k_vspline12(const double *__restrict__ t0, const double *__restrict__ t1, const long long cstride,
                                                                 const VSplineOut out, const AxisDev am, const AxisDev al, const GeoView gv,
                                                                 const int nurbs, const int g0_lo, const int gm_lo, const int Gm,
                                                                 const long long nlines, const int lpw)
{
    extern __shared__ double sp_lds[];
    constexpr int NL = GRAD ? DIM : 1;
    const int Nl = al.N, Gl = al.G, Pl = al.P, ql = al.q, Pm = am.P, Nm = am.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    double *buf = sp_lds + (size_t)wave * NC * NL * Nl;
    const long long unit = (long long)blockIdx.x * nwaves + wave;
    const long long L_lo = unit * lpw, L_hi = min(L_lo + lpw, nlines);
    for (long long L = L_lo; L < L_hi; ++L) {
        const long long plane = L / Gm;
        const int gm = gm_lo + (int)(L - plane * Gm);
        {
            const double *Vm = am.V + (size_t)gm * Pm * 2;
            const long long row = (plane * Nm + am.fa[gm / am.q]) * Nl;
            for (int i = lane; i < Nl; i += 64) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const double *s0 = t0 + c * cstride, *s1 = (GRAD && DIM == 3) ? t1 + c * cstride : nullptr;
                    double v = 0.0, dm = 0.0, d0 = 0.0;
                    for (int l = 0; l < Pm; ++l) {
                        const double x = s0[row + (long long)l * Nl + i];
                        v = fma(Vm[2 * l], x, v);
                        if (GRAD) dm = fma(Vm[2 * l + 1], x, dm);
                        if (GRAD && DIM == 3) d0 = fma(Vm[2 * l], s1[row + (long long)l * Nl + i], d0);
                    }
                    double *bc = buf + (size_t)c * NL * Nl;
                    bc[i] = v;
                    if (GRAD) bc[Nl + i] = dm;
                    if (GRAD && DIM == 3) bc[2 * Nl + i] = d0;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int g = lane; g < Gl; g += 64) {
            const double *Vl = al.V + (size_t)g * Pl * 2;
            const int fl = al.fa[g / ql];
            double v[NC], gp[NC][3];                              // parametric gradients in jet order: last, mid, axis 0
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double *b = buf + (size_t)c * NL * Nl + fl;
                v[c] = 0.0; gp[c][0] = gp[c][1] = gp[c][2] = 0.0;
                for (int l = 0; l < Pl; ++l) {
                    const double n = Vl[2 * l], x = b[l];
                    v[c] = fma(n, x, v[c]);
                    if (GRAD) {
                        gp[c][0] = fma(Vl[2 * l + 1], x, gp[c][0]);
                        gp[c][1] = fma(n, b[Nl + l], gp[c][1]);
                        if (DIM == 3) gp[c][2] = fma(n, b[2 * Nl + l], gp[c][2]);
                    }
                }
            }
            const long long idx = L * Gl + g;
#pragma unroll
            for (int c = 0; c < NC; ++c) out.o[c][idx] = v[c];
            if (GRAD) {
                int gi[3];
                if (DIM == 3) { gi[0] = g0_lo + (int)plane; gi[1] = gm; gi[2] = g; }
                else { gi[0] = gm; gi[1] = g; gi[2] = 0; }
                GradMap<DIM> M;
                gradient_map<DIM>(gv, nurbs != 0, gi, M);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    double pg[3];
                    apply_gradient_map<DIM>(M, gp[c], pg);
#pragma unroll
                    for (int r = 0; r < DIM; ++r) out.o[NC + c * DIM + r][idx] = pg[r];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// waves per block of k_spline12 such that their lines fit the 64 KB of LDS a block gets by default (0: none does); k_vspline12
// with nc components holds nc times the lines: it asks with nc * Nlast
static int spline12_waves(int dim, bool grad, int Nlast)
{
    const size_t per_wave = (size_t)(grad ? dim : 1) * Nlast * sizeof(double);
    for (int w = SP_MAXWAVES; w >= 1; w >>= 1)
        if (w * per_wave <= 64 * 1024) return w;
    return 0;
}

size_t spline_eval_workspace(const igx_patch *pt, int want_grad)
{
    const PatchDev &pd = pt->dev;
    return pd.dim == 3 ? (size_t)(want_grad ? 2 : 1) * pd.G0_loc * pd.ax[1].N * pd.ax[2].N : 0;
}

// 3D: the axis-0 expansion of the dofs into d_ws (spline_eval_workspace() doubles); *t0 / *t1: what k_spline12 and k_err12 read as
// value / axis-0 derivative planes (2D: the dofs themselves, nothing launched)
int launch_spline_axis0(hipStream_t st, const igx_patch *pt, const double *d_coeffs, int want_grad, double *d_ws, const double **t0, const double **t1)
{
    const PatchDev &pd = pt->dev;
    *t0 = d_coeffs;
    *t1 = nullptr;
    if (pd.dim != 3) return IGX_OK;
    const bool grad = want_grad != 0;
    const long long B = (long long)pd.ax[1].N * pd.ax[2].N, total = (long long)pd.G0_loc * B;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (grad) k_spline_axis0<2><<<grid, 256, 0, st>>>(d_coeffs, d_ws, pd.ax[0], pd.g0_lo, pd.G0_loc, B);
    else k_spline_axis0<1><<<grid, 256, 0, st>>>(d_coeffs, d_ws, pd.ax[0], pd.g0_lo, pd.G0_loc, B);
    IGX_HIP(hipGetLastError());
    *t0 = d_ws;
    *t1 = grad ? d_ws + total : nullptr;
    return IGX_OK;
}

// d_coeffs: N0 x N1 [x N2] dofs; d_out[0 .. dim]: resident slab arrays (value, physical gradient in jet order; the gradient only
// with want_grad); d_ws: spline_eval_workspace() doubles.  The caller has checked the patch (whole, not boxed, a spline geometry
// for the gradient).
int launch_spline_eval(hipStream_t st, const igx_patch *pt, const double *d_coeffs, int want_grad, double *const d_out[4], double *d_ws)
{
    const PatchDev &pd = pt->dev;
    const int dim = pd.dim;
    if (pd.npts_loc == 0) return IGX_OK;
    const AxisDev &am = dim == 3 ? pd.ax[1] : pd.ax[0], &al = dim == 3 ? pd.ax[2] : pd.ax[1];
    const bool grad = want_grad != 0;
    const int nw = spline12_waves(dim, grad, al.N);
    if (nw == 0) { set_error("igx_patch_eval_spline_d: %d dofs on the last axis do not fit the line buffers", al.N); return IGX_ERR_UNSUPPORTED; }
    const double *t0 = d_coeffs, *t1 = nullptr;
    if (int rc = launch_spline_axis0(st, pt, d_coeffs, want_grad, d_ws, &t0, &t1)) return rc;
    SplineOut out{};
    for (int k = 0; k < 4; ++k) out.o[k] = k == 0 || (grad && k <= dim) ? d_out[k] : nullptr;
    GeoView gv{};
    if (grad) gv = make_view(dim, pt->gax, pt->d_ctrl, pt->ncomp);
    const int nurbs = pt->geo_kind == IGX_GEO_NURBS ? 1 : 0;
    // 3D: the planes are the resident Gauss planes of axis 0 and the mid axis is whole; 2D: one plane, the mid axis IS axis 0
    const int gm_lo = dim == 3 ? 0 : pd.g0_lo, Gm = dim == 3 ? am.G : pd.G0_loc;
    const long long nlines = dim == 3 ? (long long)pd.G0_loc * Gm : Gm;
    // enough waves for the chip before a wave takes more than one line
    const int lpw = (int)std::min<long long>(8, std::max<long long>(1, nlines / 16384));
    const long long units = (nlines + lpw - 1) / lpw;
    const dim3 grid((unsigned)((units + nw - 1) / nw));
    const size_t lds = (size_t)nw * (grad ? dim : 1) * al.N * sizeof(double);
#define SPL(D_, G_) k_spline12<D_, G_><<<grid, nw * 64, lds, st>>>(t0, t1, out, am, al, gv, nurbs, pd.g0_lo, gm_lo, Gm, nlines, lpw)
    if (dim == 3) { if (grad) SPL(3, true); else SPL(3, false); }
    else { if (grad) SPL(2, true); else SPL(2, false); }
#undef SPL
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

size_t vspline_eval_workspace(const igx_patch *pt, int nc, int want_grad) { return (size_t)nc * spline_eval_workspace(pt, want_grad); }

// nc = 2 or 3 splines with component-major dofs d_coeffs (nc x N0 x N1 [x N2]); d_out[c]: values of component c, d_out[nc + c dim + r]:
// its physical partial r (want_grad); d_ws: vspline_eval_workspace() doubles.  The caller has checked the patch as for
// launch_spline_eval.  3D: the axis-0 expansion is k_spline_axis0 once per component (the scalar call's launch, the scalar call's bits).
int launch_vspline_eval(hipStream_t st, const igx_patch *pt, int nc, const double *d_coeffs, int want_grad, double *const d_out[12], double *d_ws)
{
    const PatchDev &pd = pt->dev;
    const int dim = pd.dim;
    if (pd.npts_loc == 0) return IGX_OK;
    const AxisDev &am = dim == 3 ? pd.ax[1] : pd.ax[0], &al = dim == 3 ? pd.ax[2] : pd.ax[1];
    const bool grad = want_grad != 0;
    const int nw = spline12_waves(dim, grad, nc * al.N);
    if (nw == 0) { set_error("igx_patch_eval_vspline_d: %d dofs on the last axis and %d components do not fit the line buffers", al.N, nc); return IGX_ERR_UNSUPPORTED; }
    long long ndofs = 1;
    for (int k = 0; k < dim; ++k) ndofs *= pd.ax[k].N;
    const size_t ws_c = spline_eval_workspace(pt, want_grad);
    const double *t0 = d_coeffs, *t1 = nullptr;
    long long cstride = ndofs;
    if (dim == 3) {
        for (int c = 0; c < nc; ++c) {
            const double *a = nullptr, *b = nullptr;
            if (int rc = launch_spline_axis0(st, pt, d_coeffs + (long long)c * ndofs, want_grad, d_ws + (size_t)c * ws_c, &a, &b)) return rc;
            if (c == 0) { t0 = a; t1 = b; }
        }
        cstride = (long long)ws_c;
    }
    VSplineOut out{};
    const int nout = nc * (grad ? 1 + dim : 1);
    for (int k = 0; k < nout; ++k) out.o[k] = d_out[k];
    GeoView gv{};
    if (grad) gv = make_view(dim, pt->gax, pt->d_ctrl, pt->ncomp);
    const int nurbs = pt->geo_kind == IGX_GEO_NURBS ? 1 : 0;
    const int gm_lo = dim == 3 ? 0 : pd.g0_lo, Gm = dim == 3 ? am.G : pd.G0_loc;
    const long long nlines = dim == 3 ? (long long)pd.G0_loc * Gm : Gm;
    const int lpw = (int)std::min<long long>(8, std::max<long long>(1, nlines / 16384));
    const long long units = (nlines + lpw - 1) / lpw;
    const dim3 grid((unsigned)((units + nw - 1) / nw));
    const size_t lds = (size_t)nw * nc * (grad ? dim : 1) * al.N * sizeof(double);
#define VSPL(D_, C_, G_) k_vspline12<D_, C_, G_><<<grid, nw * 64, lds, st>>>(t0, t1, cstride, out, am, al, gv, nurbs, pd.g0_lo, gm_lo, Gm, nlines, lpw)
#define VSPL_C(D_, G_) do { if (nc == 2) VSPL(D_, 2, G_); else VSPL(D_, 3, G_); } while (0)
    if (dim == 3) { if (grad) VSPL_C(3, true); else VSPL_C(3, false); }
    else { if (grad) VSPL_C(2, true); else VSPL_C(2, false); }
#undef VSPL_C
#undef VSPL
    IGX_HIP(hipGetLastError());
    return IGX_OK;
}

} // namespace igx
