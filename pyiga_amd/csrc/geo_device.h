// Device helpers shared by the geometry/fields kernels (kern_basis.hip) and the fused
// geometry + stage-A sweep (geoa.hip).
#pragma once
#include "igx_internal.h"

namespace igx {

// geometry basis restricted to the grid nodes + control net
struct GeoView {
    const double *V[3];   // [G][P][2]
    const int *fa[3];     // [G]
    int P[3], N[3];       // active count, number of control points per axis
    const double *ctrl;   // (N0,N1[,N2], nc)
    int nc;               // components incl. weight
};

// geometry: homogeneous spline value + parametric derivatives at one grid point.
// jac[c][k]: component c, derivative along GRID AXIS k (not yet reordered to x,y,z).

template <int DIM>
__device__ inline void eval_geo(const GeoView &gv, const int g[3], double val[MAX_COMP], double jac[MAX_COMP][3])
{
    const int nc = gv.nc;
    for (int c = 0; c < MAX_COMP; ++c) {
        val[c] = 0.0;
        for (int k = 0; k < 3; ++k) jac[c][k] = 0.0;
    }
    const double *V0 = gv.V[0] + (size_t)g[0] * gv.P[0] * 2;
    const double *V1 = gv.V[1] + (size_t)g[1] * gv.P[1] * 2;
    const int f0 = gv.fa[0][g[0]], f1 = gv.fa[1][g[1]];
    if (DIM == 2) {
        for (int a0 = 0; a0 < gv.P[0]; ++a0) {
            double sv[MAX_COMP], sd[MAX_COMP];
            for (int c = 0; c < MAX_COMP; ++c) sv[c] = sd[c] = 0.0;
            const double *row = gv.ctrl + ((size_t)(f0 + a0) * gv.N[1] + f1) * nc;
            for (int a1 = 0; a1 < gv.P[1]; ++a1) {
                const double n1 = V1[a1 * 2], d1 = V1[a1 * 2 + 1];
                for (int c = 0; c < nc; ++c) {
                    const double cf = row[(size_t)a1 * nc + c];
                    sv[c] += n1 * cf;
                    sd[c] += d1 * cf;
                }
            }
            const double n0 = V0[a0 * 2], d0 = V0[a0 * 2 + 1];
            for (int c = 0; c < nc; ++c) {
                val[c] += n0 * sv[c];
                jac[c][0] += d0 * sv[c];
                jac[c][1] += n0 * sd[c];
            }
        }
    } else {
        const double *V2 = gv.V[2] + (size_t)g[2] * gv.P[2] * 2;
        const int f2 = gv.fa[2][g[2]];
        for (int a0 = 0; a0 < gv.P[0]; ++a0) {
            double tv[MAX_COMP], t1[MAX_COMP], t2[MAX_COMP];
            for (int c = 0; c < MAX_COMP; ++c) tv[c] = t1[c] = t2[c] = 0.0;
            for (int a1 = 0; a1 < gv.P[1]; ++a1) {
                double sv[MAX_COMP], sd[MAX_COMP];
                for (int c = 0; c < MAX_COMP; ++c) sv[c] = sd[c] = 0.0;
                const double *row = gv.ctrl + (((size_t)(f0 + a0) * gv.N[1] + (f1 + a1)) * gv.N[2] + f2) * nc;
                for (int a2 = 0; a2 < gv.P[2]; ++a2) {
                    const double n2 = V2[a2 * 2], d2 = V2[a2 * 2 + 1];
                    for (int c = 0; c < nc; ++c) {
                        const double cf = row[(size_t)a2 * nc + c];
                        sv[c] += n2 * cf;
                        sd[c] += d2 * cf;
                    }
                }
                const double n1 = V1[a1 * 2], d1 = V1[a1 * 2 + 1];
                for (int c = 0; c < nc; ++c) {
                    tv[c] += n1 * sv[c];
                    t1[c] += d1 * sv[c];
                    t2[c] += n1 * sd[c];
                }
            }
            const double n0 = V0[a0 * 2], d0 = V0[a0 * 2 + 1];
            for (int c = 0; c < nc; ++c) {
                val[c] += n0 * tv[c];
                jac[c][0] += d0 * tv[c];
                jac[c][1] += n0 * t1[c];
                jac[c][2] += n0 * t2[c];
            }
        }
    }
}

// homogeneous value/derivatives -> physical Jacobian Jm[r][c] = dG_r / d xi_c with c in (x,y,z)
// order, i.e. c = 0 differentiates along the LAST grid axis (pyiga/bspline.py:917-921); NURBS by
// the quotient rule (pyiga/geometry.py:17-25).
template <int DIM>
__device__ inline void finish_jacobian(const double val[MAX_COMP], const double jac[MAX_COMP][3], bool nurbs,
                                       int ncomp, int nc, double Jm[MAX_COMP][3], double ev[MAX_COMP])
{
    if (nurbs) {
        // quotient rule (V'W - V W') / W^2 with ONE reciprocal: an f64 division costs ~30 VALU
        // instructions on gfx950 and the reference formula has d*d + d of them per point
        const double W = val[nc - 1];
        const double iW = 1.0 / W, iW2 = iW * iW;
        for (int r = 0; r < ncomp; ++r) {
            ev[r] = val[r] * iW;
            for (int c = 0; c < DIM; ++c) {
                const int k = DIM - 1 - c;
                Jm[r][c] = (jac[r][k] * W - val[r] * jac[nc - 1][k]) * iW2;
            }
        }
    } else {
        for (int r = 0; r < ncomp; ++r) {
            ev[r] = val[r];
            for (int c = 0; c < DIM; ++c) Jm[r][c] = jac[r][DIM - 1 - c];
        }
    }
}

// Physical Jacobian Jm[r][c] = dG_r / d xi_c with c in (x,y,z) order, i.e. c = 0 differentiates
// along the LAST grid axis (pyiga/bspline.py:917-921); NURBS by the quotient rule.
template <int DIM>
__device__ inline void physical_jacobian(const GeoView &gv, bool nurbs, const int g[3], int ncomp,
                                         double Jm[MAX_COMP][3], double ev[MAX_COMP])
{
    double val[MAX_COMP], jac[MAX_COMP][3];
    eval_geo<DIM>(gv, g, val, jac);
    finish_jacobian<DIM>(val, jac, nurbs, ncomp, gv.nc, Jm, ev);
}

// Physical gradient of a function from its PARAMETRIC gradient gp in jet order (last grid axis first) at Gauss point gi:
// D_r w = sum_c (d xi_c / d x_r) Dhat_c w, the inverse of Jm[r][c] = d G_r / d xi_c.  One text for the spline evaluation
// (kern_spline.hip) and the error sums (kern_quad.hip): the two compute the same gradient.
template <int DIM>
__device__ __forceinline__ void physical_gradient(const GeoView &gv, bool nurbs, const int gi[3], const double gp[3], double pg[3])
{
    double Jm[MAX_COMP][3], ev[MAX_COMP];
    physical_jacobian<DIM>(gv, nurbs, gi, DIM, Jm, ev);
    if (DIM == 2) {
        const double inv = 1.0 / (Jm[0][0] * Jm[1][1] - Jm[0][1] * Jm[1][0]);
        // JI = inv * [[J11, -J01], [-J10, J00]]; D_r = sum_c JI[c][r] gp[c]
        pg[0] = inv * (Jm[1][1] * gp[0] - Jm[1][0] * gp[1]);
        pg[1] = inv * (Jm[0][0] * gp[1] - Jm[0][1] * gp[0]);
    } else {
        const double t[9] = {Jm[0][0], Jm[0][1], Jm[0][2], Jm[1][0], Jm[1][1], Jm[1][2], Jm[2][0], Jm[2][1], Jm[2][2]};
        const double t3 = t[4] * t[8] - t[5] * t[7];
        const double t4 = t[3] * t[8] - t[5] * t[6];
        const double t5 = t[3] * t[7] - t[4] * t[6];
        const double inv = 1.0 / ((t[0] * t3 - t[1] * t4) + t[2] * t5);
        double JI[9];                               // JI[3 c + r] = d xi_c / d x_r (fields_form: T[1 + c][1 + r])
        JI[0] = inv * t3;
        JI[1] = inv * -(t[1] * t[8] - t[2] * t[7]);
        JI[2] = inv * (t[1] * t[5] - t[2] * t[4]);
        JI[3] = inv * -t4;
        JI[4] = inv * (t[0] * t[8] - t[2] * t[6]);
        JI[5] = inv * -(t[0] * t[5] - t[2] * t[3]);
        JI[6] = inv * t5;
        JI[7] = inv * -(t[0] * t[7] - t[1] * t[6]);
        JI[8] = inv * (t[0] * t[4] - t[1] * t[3]);
#pragma unroll
        for (int r = 0; r < 3; ++r) pg[r] = (JI[r] * gp[0] + JI[3 + r] * gp[1]) + JI[6 + r] * gp[2];
    }
}

// Second-derivative tables of the geometry basis at the grid nodes, beside the GeoView (igx_patch_residual_sums_d): the tables
// of launch_basis_tables' plain output, D2[k][l * G[k] + g] = second derivative of active function l of axis k at node g.
struct GeoView2 {
    const double *D2[3];
    int G[3];
};

// geometry up to second order at one grid point: per component c (homogeneous: the weight is component DIM of a NURBS map)
//   val[c], d1[c][k] = d / d xi_k, d2[c][.] = d^2 / d xi_a d xi_b in the order (00, 01, 11) / (00, 01, 02, 11, 12, 22), GRID axes.
// One component at a time: 19 partial sums live instead of 19 per component.
template <int DIM>
__device__ inline void eval_geo2(const GeoView &gv, const GeoView2 &g2, bool nurbs, const int g[3], double val[DIM + 1], double d1[DIM + 1][3],
                                 double d2[DIM + 1][6])
{
    const int nc = gv.nc;
    const double *V0 = gv.V[0] + (size_t)g[0] * gv.P[0] * 2, *V1 = gv.V[1] + (size_t)g[1] * gv.P[1] * 2;
    const double *D0 = g2.D2[0] + g[0], *D1 = g2.D2[1] + g[1];
    const int f0 = gv.fa[0][g[0]], f1 = gv.fa[1][g[1]];
#pragma unroll
    for (int c = 0; c <= DIM; ++c) {
        if (c == DIM && !nurbs) {
            val[c] = 1.0;
            for (int k = 0; k < 3; ++k) d1[c][k] = 0.0;
            for (int k = 0; k < 6; ++k) d2[c][k] = 0.0;
            continue;
        }
        if (DIM == 2) {
            double v = 0.0, a0 = 0.0, a1 = 0.0, h00 = 0.0, h01 = 0.0, h11 = 0.0;
            for (int i0 = 0; i0 < gv.P[0]; ++i0) {
                const double *row = gv.ctrl + ((size_t)(f0 + i0) * gv.N[1] + f1) * nc + c;
                double sv = 0.0, sd = 0.0, sdd = 0.0;
                for (int i1 = 0; i1 < gv.P[1]; ++i1) {
                    const double cf = row[(size_t)i1 * nc];
                    sv = fma(V1[i1 * 2], cf, sv);
                    sd = fma(V1[i1 * 2 + 1], cf, sd);
                    sdd = fma(D1[(size_t)i1 * g2.G[1]], cf, sdd);
                }
                const double n0 = V0[i0 * 2], e0 = V0[i0 * 2 + 1], ee0 = D0[(size_t)i0 * g2.G[0]];
                v = fma(n0, sv, v);
                a0 = fma(e0, sv, a0);
                a1 = fma(n0, sd, a1);
                h00 = fma(ee0, sv, h00);
                h01 = fma(e0, sd, h01);
                h11 = fma(n0, sdd, h11);
            }
            val[c] = v;
            d1[c][0] = a0; d1[c][1] = a1; d1[c][2] = 0.0;
            d2[c][0] = h00; d2[c][1] = h01; d2[c][2] = h11; d2[c][3] = d2[c][4] = d2[c][5] = 0.0;
        } else {
            const double *V2 = gv.V[2] + (size_t)g[2] * gv.P[2] * 2, *D2 = g2.D2[2] + g[2];
            const int f2 = gv.fa[2][g[2]];
            double v = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0;
            for (int i0 = 0; i0 < gv.P[0]; ++i0) {
                double tv = 0.0, t1 = 0.0, t2 = 0.0, t11 = 0.0, t12 = 0.0, t22 = 0.0;
                for (int i1 = 0; i1 < gv.P[1]; ++i1) {
                    const double *row = gv.ctrl + (((size_t)(f0 + i0) * gv.N[1] + (f1 + i1)) * gv.N[2] + f2) * nc + c;
                    double sv = 0.0, sd = 0.0, sdd = 0.0;
                    for (int i2 = 0; i2 < gv.P[2]; ++i2) {
                        const double cf = row[(size_t)i2 * nc];
                        sv = fma(V2[i2 * 2], cf, sv);
                        sd = fma(V2[i2 * 2 + 1], cf, sd);
                        sdd = fma(D2[(size_t)i2 * g2.G[2]], cf, sdd);
                    }
                    const double n1 = V1[i1 * 2], e1 = V1[i1 * 2 + 1], ee1 = D1[(size_t)i1 * g2.G[1]];
                    tv = fma(n1, sv, tv);
                    t1 = fma(e1, sv, t1);
                    t2 = fma(n1, sd, t2);
                    t11 = fma(ee1, sv, t11);
                    t12 = fma(e1, sd, t12);
                    t22 = fma(n1, sdd, t22);
                }
                const double n0 = V0[i0 * 2], e0 = V0[i0 * 2 + 1], ee0 = D0[(size_t)i0 * g2.G[0]];
                v = fma(n0, tv, v);
                a0 = fma(e0, tv, a0);
                a1 = fma(n0, t1, a1);
                a2 = fma(n0, t2, a2);
                h00 = fma(ee0, tv, h00);
                h01 = fma(e0, t1, h01);
                h02 = fma(e0, t2, h02);
                h11 = fma(n0, t11, h11);
                h12 = fma(n0, t12, h12);
                h22 = fma(n0, t22, h22);
            }
            val[c] = v;
            d1[c][0] = a0; d1[c][1] = a1; d1[c][2] = a2;
            d2[c][0] = h00; d2[c][1] = h01; d2[c][2] = h02; d2[c][3] = h11; d2[c][4] = h12; d2[c][5] = h22;
        }
    }
}

// index of the pair (a, b), a <= b, in the packed upper triangle of eval_geo2
template <int DIM>
__device__ __forceinline__ constexpr int sym_index(int a, int b)
{
    return DIM == 2 ? a + b : (a == 0 ? b : a + b + 1);
}

// The coefficients of the physical Laplacian in parametric derivatives at one point:
//     Lap u = sum_{c <= d} K[cd] D_c D_d u^ (off-diagonal entries doubled by the caller) + sum_c b[c] D_c u^
// with JI = J^-1 (JI[c][r] = d xi_c / d x_r), K = JI JI^t and b_c = -sum_m JI[c][m] sum_{e,u} H2[m][e][u] K[e][u], H2 the second
// parametric derivatives of the map (the trace of pyiga/vform.py:609-625's Christoffel term).  All parametric indices in JET
// order: c = 0 is the LAST grid axis.  NURBS: second-order quotient rule with ONE reciprocal,
//     x = A / w,  x_a = (A_a - w_a x) / w,  x_ab = (A_ab - w_a x_b - w_b x_a - w_ab x) / w.
// K packed as eval_geo2 packs (00, 01[, 02], 11[, 12, 22]).
template <int DIM>
__device__ inline void laplace_coefficients(const GeoView &gv, const GeoView2 &g2, bool nurbs, const int gi[3], double K[6], double b[3])
{
    double val[DIM + 1], d1[DIM + 1][3], d2[DIM + 1][6];
    eval_geo2<DIM>(gv, g2, nurbs, gi, val, d1, d2);
    // physical first / second derivatives along GRID axes
    double X1[DIM][DIM], X2[DIM][DIM * (DIM + 1) / 2];
    if (nurbs) {
        const double iw = 1.0 / val[DIM];
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
            const double x = val[r] * iw;
#pragma unroll
            for (int a = 0; a < DIM; ++a) X1[r][a] = (d1[r][a] - d1[DIM][a] * x) * iw;
#pragma unroll
            for (int a = 0; a < DIM; ++a)
#pragma unroll
                for (int bb = a; bb < DIM; ++bb) {
                    const int t = sym_index<DIM>(a, bb);
                    X2[r][t] = (((d2[r][t] - d1[DIM][a] * X1[r][bb]) - d1[DIM][bb] * X1[r][a]) - d2[DIM][t] * x) * iw;
                }
        }
    } else {
#pragma unroll
        for (int r = 0; r < DIM; ++r) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) X1[r][a] = d1[r][a];
#pragma unroll
            for (int t = 0; t < DIM * (DIM + 1) / 2; ++t) X2[r][t] = d2[r][t];
        }
    }
    // jet order: parametric index c <-> grid axis DIM - 1 - c
    double JI[DIM][DIM];
    if (DIM == 2) {
        const double J00 = X1[0][1], J01 = X1[0][0], J10 = X1[1][1], J11 = X1[1][0];
        const double inv = 1.0 / (J00 * J11 - J01 * J10);
        JI[0][0] = inv * J11; JI[0][1] = inv * -J01;
        JI[1][0] = inv * -J10; JI[1][1] = inv * J00;
    } else {
        const double t[9] = {X1[0][2], X1[0][1], X1[0][0], X1[1][2], X1[1][1], X1[1][0], X1[2][2], X1[2][1], X1[2][0]};
        const double t3 = t[4] * t[8] - t[5] * t[7];
        const double t4 = t[3] * t[8] - t[5] * t[6];
        const double t5 = t[3] * t[7] - t[4] * t[6];
        const double inv = 1.0 / ((t[0] * t3 - t[1] * t4) + t[2] * t5);
        JI[0][0] = inv * t3;
        JI[0][1] = inv * -(t[1] * t[8] - t[2] * t[7]);
        JI[0][2] = inv * (t[1] * t[5] - t[2] * t[4]);
        JI[1][0] = inv * -t4;
        JI[1][1] = inv * (t[0] * t[8] - t[2] * t[6]);
        JI[1][2] = inv * -(t[0] * t[5] - t[2] * t[3]);
        JI[2][0] = inv * t5;
        JI[2][1] = inv * -(t[0] * t[7] - t[1] * t[6]);
        JI[2][2] = inv * (t[0] * t[4] - t[1] * t[3]);
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c)
#pragma unroll
        for (int d = c; d < DIM; ++d) {
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < DIM; ++r) s = fma(JI[c][r], JI[d][r], s);
            K[sym_index<DIM>(c, d)] = s;
        }
    // s_m = sum_{e,u} H2[m][e][u] K[e][u]; jet pair (e, u) is grid pair (DIM-1-u, DIM-1-e)
    double sm[DIM];
#pragma unroll
    for (int m = 0; m < DIM; ++m) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < DIM; ++e)
#pragma unroll
            for (int u = e; u < DIM; ++u) {
                const double h = X2[m][sym_index<DIM>(DIM - 1 - u, DIM - 1 - e)], k = K[sym_index<DIM>(e, u)];
                s = fma(e == u ? h : 2.0 * h, k, s);
            }
        sm[m] = s;
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < DIM; ++m) s = fma(JI[c][m], sm[m], s);
        b[c] = -s;
    }
}

// quadrature fields of one point from its Jacobian (row-major t[]): f[0] = W for the mass form, the upper
// triangle of  W * JacInv JacInv^T  (row-major) for the stiffness form.  Returns the number of fields.
template <int DIM>
__device__ inline int fields_values(const double t[9], double GW, int kind, double f[6])
{
    if (DIM == 2) {
        const double det = t[0] * t[3] - t[1] * t[2];
        const double W = GW * fabs(det);
        if (kind == IGX_MASS) { f[0] = W; return 1; }
        const double inv = 1.0 / det;
        const double J0 = inv * t[3], J1 = inv * -t[1], J2 = inv * -t[2], J3 = inv * t[0];
        f[0] = W * (J0 * J0 + J1 * J1);
        f[1] = W * (J0 * J2 + J1 * J3);
        f[2] = W * (J2 * J2 + J3 * J3);
        return 3;
    } else {
        const double t3 = t[4] * t[8] - t[5] * t[7];
        const double t4 = t[3] * t[8] - t[5] * t[6];
        const double t5 = t[3] * t[7] - t[4] * t[6];
        const double det = (t[0] * t3 - t[1] * t4) + t[2] * t5;
        const double W = GW * fabs(det);
        if (kind == IGX_MASS) { f[0] = W; return 1; }
        const double inv = 1.0 / det;
        double JI[9];
        JI[0] = inv * t3;
        JI[1] = inv * -(t[1] * t[8] - t[2] * t[7]);
        JI[2] = inv * (t[1] * t[5] - t[2] * t[4]);
        JI[3] = inv * -t4;
        JI[4] = inv * (t[0] * t[8] - t[2] * t[6]);
        JI[5] = inv * -(t[0] * t[5] - t[2] * t[3]);
        JI[6] = inv * t5;
        JI[7] = inv * -(t[0] * t[7] - t[1] * t[6]);
        JI[8] = inv * (t[0] * t[4] - t[1] * t[3]);
        f[0] = W * ((JI[0] * JI[0] + JI[1] * JI[1]) + JI[2] * JI[2]);
        f[1] = W * ((JI[0] * JI[3] + JI[1] * JI[4]) + JI[2] * JI[5]);
        f[2] = W * ((JI[0] * JI[6] + JI[1] * JI[7]) + JI[2] * JI[8]);
        f[3] = W * ((JI[3] * JI[3] + JI[4] * JI[4]) + JI[5] * JI[5]);
        f[4] = W * ((JI[3] * JI[6] + JI[4] * JI[7]) + JI[5] * JI[8]);
        f[5] = W * ((JI[6] * JI[6] + JI[7] * JI[7]) + JI[8] * JI[8]);
        return 6;
    }
}

// ... stored as fields[f*stride + pt]
template <int DIM>
__device__ inline void fields_from_jac(const double t[9], double GW, int kind, double *fields, long long stride, long long pt)
{
    double f[6];
    const int nf = fields_values<DIM>(t, GW, kind, f);
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (k < nf) fields[k * stride + pt] = f[k];
}

// Fields of the convection-diffusion form (3D): c*B (upper triangle, as stiffness) and
// beta_a = W * sum_r JacInv[a][r] * b_r with b = (y, -x, 1) at the physical point ev.
__device__ inline void fields_convdiff(const double t[9], double GW, const double ev[MAX_COMP], double c,
                                       double *fields, long long stride, long long pt)
{
    const double t3 = t[4] * t[8] - t[5] * t[7];
    const double t4 = t[3] * t[8] - t[5] * t[6];
    const double t5 = t[3] * t[7] - t[4] * t[6];
    const double det = (t[0] * t3 - t[1] * t4) + t[2] * t5;
    const double W = GW * fabs(det);
    const double inv = 1.0 / det;
    double JI[9];
    JI[0] = inv * t3;
    JI[1] = inv * -(t[1] * t[8] - t[2] * t[7]);
    JI[2] = inv * (t[1] * t[5] - t[2] * t[4]);
    JI[3] = inv * -t4;
    JI[4] = inv * (t[0] * t[8] - t[2] * t[6]);
    JI[5] = inv * -(t[0] * t[5] - t[2] * t[3]);
    JI[6] = inv * t5;
    JI[7] = inv * -(t[0] * t[7] - t[1] * t[6]);
    JI[8] = inv * (t[0] * t[4] - t[1] * t[3]);
    const double cW = c * W;
    fields[pt] = cW * ((JI[0] * JI[0] + JI[1] * JI[1]) + JI[2] * JI[2]);
    fields[stride + pt] = cW * ((JI[0] * JI[3] + JI[1] * JI[4]) + JI[2] * JI[5]);
    fields[2 * stride + pt] = cW * ((JI[0] * JI[6] + JI[1] * JI[7]) + JI[2] * JI[8]);
    fields[3 * stride + pt] = cW * ((JI[3] * JI[3] + JI[4] * JI[4]) + JI[5] * JI[5]);
    fields[4 * stride + pt] = cW * ((JI[3] * JI[6] + JI[4] * JI[7]) + JI[5] * JI[8]);
    fields[5 * stride + pt] = cW * ((JI[6] * JI[6] + JI[7] * JI[7]) + JI[8] * JI[8]);
    const double b0 = ev[1], b1 = -ev[0], b2 = 1.0;
    fields[6 * stride + pt] = W * ((JI[0] * b0 + JI[1] * b1) + JI[2] * b2);
    fields[7 * stride + pt] = W * ((JI[3] * b0 + JI[4] * b1) + JI[5] * b2);
    fields[8 * stride + pt] = W * ((JI[6] * b0 + JI[7] * b1) + JI[8] * b2);
}

// IGX_FORM: parametric jet coefficients  M = W * T P T^t,  T = diag(1, JacInv)  (JacInv[a][r] = d xi_a / d x_r),
// so that  sum_rs P_rs D_r v D_s u  (physical jets)  =  sum_ab M_ab Dhat_a v Dhat_b u  (parametric jets).
// Only the terms listed in form_ab are stored (field t <-> form_ab[t] = 4 a + b).
// form_par: the coefficients are parametric already (igx_patch_set_pform): field k = Gauss weight * coefficient k.
template <int DIM>
__device__ inline void fields_form(const double t[9], double GW, const FormView &fv, const int form_n, const int *form_ab, const int form_par,
                                   double *fields, long long stride, long long pt)
{
    if (form_par) {
        for (int k = 0; k < form_n; ++k) fields[(long long)k * stride + pt] = GW * fv.c[(long long)k * stride + pt];
        return;
    }
    constexpr int NJ = DIM + 1;
    double T[4][4];
    for (int r = 0; r < 4; ++r)
        for (int s = 0; s < 4; ++s) T[r][s] = 0.0;
    T[0][0] = 1.0;
    double det;
    if (DIM == 2) {
        det = t[0] * t[3] - t[1] * t[2];
        const double inv = 1.0 / det;
        T[1][1] = inv * t[3]; T[1][2] = inv * -t[1];
        T[2][1] = inv * -t[2]; T[2][2] = inv * t[0];
    } else {
        const double t3 = t[4] * t[8] - t[5] * t[7];
        const double t4 = t[3] * t[8] - t[5] * t[6];
        const double t5 = t[3] * t[7] - t[4] * t[6];
        det = (t[0] * t3 - t[1] * t4) + t[2] * t5;
        const double inv = 1.0 / det;
        T[1][1] = inv * t3;
        T[1][2] = inv * -(t[1] * t[8] - t[2] * t[7]);
        T[1][3] = inv * (t[1] * t[5] - t[2] * t[4]);
        T[2][1] = inv * -t4;
        T[2][2] = inv * (t[0] * t[8] - t[2] * t[6]);
        T[2][3] = inv * -(t[0] * t[5] - t[2] * t[3]);
        T[3][1] = inv * t5;
        T[3][2] = inv * -(t[0] * t[7] - t[1] * t[6]);
        T[3][3] = inv * (t[0] * t[4] - t[1] * t[3]);
    }
    const double W = GW * fabs(det);
    double P[4][4];
#pragma unroll
    for (int r = 0; r < NJ; ++r)
#pragma unroll
        for (int s = 0; s < NJ; ++s) {
            const int sl = fv.slot[4 * r + s];
            P[r][s] = sl >= 0 ? fv.c[(long long)sl * stride + pt] : 0.0;
        }
    double TP[4][4];                                   // T P: rows of T act on the test index
#pragma unroll
    for (int a = 0; a < NJ; ++a)
#pragma unroll
        for (int s = 0; s < NJ; ++s) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < NJ; ++r) v = fma(T[a][r], P[r][s], v);
            TP[a][s] = v;
        }
    for (int k = 0; k < form_n; ++k) {
        const int a = form_ab[k] >> 2, b = form_ab[k] & 3;
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < NJ; ++s) v = fma(TP[a][s], T[b][s], v);
        fields[(long long)k * stride + pt] = W * v;
    }
}

inline GeoView make_view(int dim, const GeoAxis gax[3], const double *d_ctrl, int nc)
{
    GeoView gv{};
    for (int k = 0; k < 3; ++k) {
        gv.V[k] = k < dim ? gax[k].d_V : nullptr;
        gv.fa[k] = k < dim ? gax[k].d_fa : nullptr;
        gv.P[k] = k < dim ? gax[k].P : 1;
        gv.N[k] = k < dim ? gax[k].N : 1;
    }
    gv.ctrl = d_ctrl;
    gv.nc = nc;
    return gv;
}

} // namespace igx
