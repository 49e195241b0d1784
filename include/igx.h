/*
 * igx.h -- C ABI of libigx: MI355X (gfx950) tensor-product IgA assembly.
 *
 * This is the drop-in boundary for the hot path of c-f-h/pyiga
 *     pyiga.assemble.stiffness()/mass()  with a geometry map
 * (SURVEY.md section 8b).  Plain pointers and sizes only; no C++ or torch types.
 * Every entry point returns 0 on success and a non-zero code on failure
 * (message via igx_last_error()); nothing throws across the ABI.  All
 * `const double*` / `const size_t*` arguments are HOST pointers unless the name
 * starts with `d_`.  Host output buffers are allocated by the caller.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   igx_active_deriv / igx_find_spans  <- pyiga/bspline_cy.pyx:13-27,126-145
 *   igx_patch_create                   <- *Assembler{2,3}D.__init__
 *                                         pyiga/assemblers.pyx:38-80,186-228,1170-1217,1336-1383
 *                                         (quadrature.py:3-23, bspline.py:129-136,629-660,
 *                                          geometry.py:17-25,116-123, tensor.py:97-128,
 *                                          precompute_fields assemblers.pyx:86-110,234-275,1223-1249,1389-1449)
 *   igx_grid_jacobian / igx_grid_eval  <- BSplineFunc/NurbsFunc.grid_jacobian/grid_eval
 *                                         pyiga/bspline.py:874-921, pyiga/geometry.py:103-123
 *   igx_pattern                        <- MLStructure.from_kvs + nonzero
 *                                         pyiga/mlmatrix.py:59-65,113-130,420-440; mlmatrix_cy.pyx:189-289
 *                                         (emits canonical CSR directly instead of COO pairs)
 *   igx_entries                        <- BaseAssembler{2,3}D.multi_entries / entry
 *                                         pyiga/genericasm.pxi:353-436,677-758
 *                                         (entry_impl + combine, assemblers.pyx:116-172,281-349,1255-1322,1455-1540)
 *   igx_patch_set_coeff + IGX_CONVDIFF <- the assembler pyiga.compile.compile_vform generates for the form
 *                                         (pyiga/assemble.py:837-897, pyiga/codegen/cython.py:325-387,673-701)
 *   igx_patch_set_form + IGX_FORM      <- assemble.assemble(<form string>, ...) for scalar forms that are bilinear in
 *                                         (u, grad u) x (v, grad v): pyiga/assemble.py:837-897, pyiga/vform.py:1804-1885
 *   igx_load_vector                    <- inner_products / *FunctionalAssembler*.assemble_vector
 *                                         pyiga/assemble.py:288-340, pyiga/assemblers.pyx:883-1156,2204-2500,
 *                                         pyiga/genericasm.pxi:438-456,762-778
 *   igx_assemble                       <- assemble_entries(asm, symmetric=True)
 *                                         pyiga/assemble.py:703-754 (multi_entries + COO->CSR + mirror)
 *   igx_multipatch_*                   <- Multipatch.assemble_system: A += X_p @ A_p @ X_p.T, b += X_p @ b_p
 *                                         pyiga/assemble.py:1340-1370 (global pattern and sums on the device)
 *   igx_solver_* / igx_kron_apply_d    <- RestrictedLinearSystem + make_solver / cg, fastdiag_solver, KroneckerOperator
 *                                         pyiga/assemble.py:571-652, pyiga/solvers.py:17-42, pyiga/operators.py:60-86,
 *                                         pyiga/approx.py:62-96 (one patch, matrix values never leave the device)
 *   igx_solver_*_parabolic / _dirk_*   <- crank_nicolson, sdirk3, esdirk34, ... (dirk_step, constant steps)
 *                                         pyiga/solvers.py:366-473 (linear M u' = f - K u, one patch, on the device)
 *   igx_solver_set_stepper / _step_*   <- sdirk21 .. esdirk34 with adaptive steps, ros3p .. rosi2p1 (rosenbrock_step)
 *                                         pyiga/solvers.py:430-435, 475-534, 684-939 (a session of attempts)
 *   igx_solver_eig_*                   <- scipy.sparse.linalg.eigsh / lobpcg on the two host matrices of a patch
 *                                         (the lowest eigenpairs of K x = lam M x; block LOBPCG, the pieces on the device)
 *   igx_solver_take_mass + _eig_*      <- the same on assemble(vector form, layout='blocked') and block_diag([mass] * nc):
 *                                         elastic vibration, K x = lam (I (x) M) x on a block solver (igx_solver_create_block)
 */
#ifndef IGX_H
#define IGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGX_VERSION 101            /* 0.1.1: igx_patch_desc.box_lo / box_hi */
#define IGX_MAX_DIM 3
#define IGX_MAX_DEGREE 15          /* basis evaluation / entry-wise kernels */
#define IGX_MAX_SF_DEGREE 7        /* sum-factorised fast path */

typedef struct igx_ctx igx_ctx;       /* one per GPU: device id + HIP stream */
typedef struct igx_patch igx_patch;   /* device-resident state of one assembler */
typedef struct igx_multipatch igx_multipatch;   /* global CSR of several patches glued at their interfaces */

enum { IGX_MASS = 0, IGX_STIFFNESS = 1,
       /* (inner(c*grad(u),grad(v)) + inner((x[1],-x[0],1.0),grad(u))*v)*dx -- the custom (vform) case of
          BASELINE config 5, non-symmetric, 3D only; c is set with igx_patch_set_coeff */
       IGX_CONVDIFF = 2,
       /* general scalar bilinear form in the first-order jets of u and v (2D: r,s = 0..2):
            a(u,v) = integral of  sum_{r,s=0..3} P_rs(x) * D_r v * D_s u ,   D_0 = identity, D_1..3 = d/dx, d/dy, d/dz (physical)
          P_rs are coefficient fields set with igx_patch_set_form: the block r,s >= 1 is a diffusion tensor
          (inner(dot(K,grad(u)),grad(v)): P = K), row 0 a convection vector (inner(b,grad(u))*v), column 0 its
          adjoint (u*inner(b,grad(v))), P_00 a reaction coefficient (c*u*v).  Non-symmetric.  What the
          reference compiles from a form string (pyiga/vform.py, pyiga/codegen/cython.py) for this class. */
       IGX_FORM = 3 };
enum { IGX_GEO_BSPLINE = 0, IGX_GEO_NURBS = 1, IGX_GEO_JACOBIAN = 2 };
/* algorithm selector for igx_assemble */
enum { IGX_ALGO_AUTO = 0,      /* sum-factorised when the patch supports it, else entry-wise */
       IGX_ALGO_ENTRYWISE = 1, /* one thread per matrix entry, the reference's own summation order */
       IGX_ALGO_SUMFACT = 2 }; /* global sum factorisation (stage kernels) */

enum { IGX_OK = 0, IGX_ERR_ARG = 1, IGX_ERR_HIP = 2, IGX_ERR_UNSUPPORTED = 3, IGX_ERR_NOMEM = 4,
       IGX_ERR_NORTC = 5,      /* an entry point that compiles at run time, on a box without libhiprtc: take the sampled-array path */
       IGX_ERR_COMPILE = 6 };  /* the expression handed to the run-time compiler did not compile (igx_last_error has the log) */

/* Knot vectors are in the reference's (z, y, x) order: axis 0 is the slowest dof index. */
typedef struct {
    int32_t dim;                       /* 2 or 3 */
    int32_t p[IGX_MAX_DIM];            /* spline degree per axis */
    int32_t kv_len[IGX_MAX_DIM];       /* number of knots per axis */
    const double *kv[IGX_MAX_DIM];     /* open knot vectors */

    int32_t geo_kind;                  /* IGX_GEO_* */
    int32_t geo_p[IGX_MAX_DIM];        /* geometry degrees (BSPLINE/NURBS) */
    int32_t geo_kv_len[IGX_MAX_DIM];
    const double *geo_kv[IGX_MAX_DIM];
    const double *ctrl;                /* control net, C order, shape (Ng0,..,Ng{d-1}, dim [+1 weight, premultiplied]) */
    const double *jac;                 /* IGX_GEO_JACOBIAN: (G0,..,G{d-1}, d, d), last axis = d/d(x,y,z) */

    int32_t nqp;                       /* Gauss points per span; 0 -> max(p)+1 as in the reference */
    const double *gauss_x;             /* optional nqp nodes on [-1,1] (NULL -> built-in Gauss-Legendre) */
    const double *gauss_w;             /* optional nqp weights */

    /* Row slab for multi-GPU: this patch owns the dof planes row0_lo <= i0 < row0_hi of axis 0
       (row0_hi = 0 means "all").  Only those CSR rows are produced. */
    int32_t row0_lo, row0_hi;

    /* Span box for on-demand assemblers (pyiga/codegen/cython.py:541-559, callers pyiga/_hdiscr.py:37-56,204-209): the
       geometry-dependent fields are kept only on the spans box_lo[k] <= s < box_hi[k] of every axis (all box_hi zero = whole
       patch).  A boxed patch serves igx_entries / igx_entries_d for pairs whose common support lies inside the box (others:
       NaN) and nothing else; IGX_GEO_JACOBIAN arrays and sampled coefficients are then given on the Gauss grid of the BOX.
       Present since igx_version() >= 101. */
    int32_t box_lo[IGX_MAX_DIM], box_hi[IGX_MAX_DIM];
} igx_patch_desc;

typedef struct {
    int32_t dim, nqp;
    int32_t ndofs[IGX_MAX_DIM], nspans[IGX_MAX_DIM], ngauss[IGX_MAX_DIM];
    int64_t nrows_total;               /* prod(ndofs) */
    int64_t row_lo, row_hi;            /* owned global rows [row_lo, row_hi) */
    int64_t nnz;                       /* nonzeros in the owned rows */
    int64_t nnz_offset;                /* global indptr[row_lo] */
    int64_t nelem_owned;               /* elements attributed to this slab (for throughput) */
    int32_t sumfact_ok;                /* 1 if the fast path supports this patch */
    int32_t reserved;
} igx_patch_info;

/* Device time of the last igx_assemble (HIP events on the ctx stream), milliseconds.  total_ms is always measured.  The
   per-kernel fields need events between the kernels and a marker costs ~5 us of stream time: they are recorded for 3D
   patches of >= 2^24 Gauss points (kernels of milliseconds) or when the patch was created under IGX_STAGE_EVENTS=1, and
   are 0 otherwise (a single-launch 2D assembly reports its one kernel as stage1_ms = total_ms). */
typedef struct {
    float total_ms;
    float fields_ms, stage0_ms, stage1_ms, final_ms, entry_ms;
    int32_t algo_used;                 /* IGX_ALGO_ENTRYWISE / IGX_ALGO_SUMFACT; 3 after igx_load_vector (total_ms = its contractions), 4 / 5: igx_patch_eval_spline_d / _exprs_inputs_d, 6: igx_patch_quad_sums_d / _error_sums_d, 7: igx_patch_add_face / _host (total_ms = the add) */
    int32_t n_launches;
} igx_timing;

/* kernels the last igx_assemble(.., IGX_ALGO_SUMFACT) of a patch ran (igx_patch_last_path) */
#define IGX_PATH_GEOA    1   /* geometry + axis-0 sweep fused (k_geoA): timing.fields_ms ~ 0, stage0_ms = k_geoA */
#define IGX_PATH_FUSED   2   /* sweep + final stage fused (k_bf): timing.stage1_ms = k_bf */
#define IGX_PATH_MIRROR  4   /* upper triangle by the transposing mirror pass: timing.final_ms = k_mirror */
#define IGX_PATH_SINGLE  8   /* 2D mass / stiffness in ONE launch (k_single2d: fields, sweep and contraction in LDS): timing.stage1_ms */
#define IGX_PATH_BOTH   32   /* the fused stage wrote both triangles of a symmetric form itself (k_bf3): no mirror pass; timing.stage1_ms = k_bf3 */
#define IGX_PATH_BF3    64   /* the fused stage ran as k_bf3 (fused3.hip: entry rings per line, store duty on the sweeper waves) */
#define IGX_PATH_TWIN  128   /* repeated knots on the last axis: the chain ran on the patch with mid and last axis exchanged, k_bf3 stored to this patch's layout */
#define IGX_PATH_GEOA_ROT 256 /* k_geoA's pair-product sweep kept its pair window in place and rotated the register names (single interior knots on axis 0) */
#define IGX_PATH_KRON   16   /* separable geometry: 2D matrices of the cross-section expanded by k_kron3 (igx_assemble_kron3): timing.final_ms */

int         igx_version(void);
const char *igx_last_error(void);

igx_ctx *igx_create(int device_id);                 /* NULL on failure */
void     igx_destroy(igx_ctx *ctx);
int      igx_sync(igx_ctx *ctx);
void    *igx_stream(igx_ctx *ctx);                  /* hipStream_t of this context */

/* --- B-spline evaluation (bspline_cy.pyx) ------------------------------------------------- */
/* out has shape (numderiv+1, p+1, nu), C order, exactly like pyiga.bspline_cy.active_deriv */
int igx_active_deriv(igx_ctx *ctx, const double *kv, int kv_len, int p,
                     const double *u, size_t nu, int numderiv, double *out);
/* spans[i] = pyx_findspan(kv, p, u[i]) */
int igx_find_spans(igx_ctx *ctx, const double *kv, int kv_len, int p,
                   const double *u, size_t nu, int64_t *spans);

/* --- geometry on a tensor grid (bspline.py:874-921, geometry.py:103-123) ------------------- */
/* desc uses only dim, geo_kind (BSPLINE/NURBS), geo_p, geo_kv_len, geo_kv, ctrl.
   ncomp = number of output components (geo.dim).  jac_out: (n0,..,n{d-1}, ncomp, d); eval_out:
   (n0,..,n{d-1}, ncomp).  Either output may be NULL. */
int igx_grid_jacobian(igx_ctx *ctx, const igx_patch_desc *desc, int ncomp,
                      const double *const grid[IGX_MAX_DIM], const int32_t ngrid[IGX_MAX_DIM],
                      double *jac_out, double *eval_out);

/* --- patch = assembler state on the device -------------------------------------------------- */
igx_patch *igx_patch_create(igx_ctx *ctx, const igx_patch_desc *desc);   /* NULL on failure */
void       igx_patch_destroy(igx_patch *patch);
int        igx_patch_get_info(const igx_patch *patch, igx_patch_info *info);

/* Scalar coefficient field of IGX_CONVDIFF on the FULL tensor Gauss grid (G0 x G1 x G2, C order, host
   pointer; what pyiga.utils.grid_eval_transformed(diff_coeff, gaussgrid, geo) returns).  Copied. */
int igx_patch_set_coeff(igx_patch *patch, const double *coeff);
/* The same coefficient given as an affine function of the PHYSICAL coordinates, c(x) = c[0] + c[1] x + c[2] y + c[3] z:
   evaluated on the device through the geometry map, nothing is sampled or shipped by the host. */
int igx_patch_set_coeff_affine(igx_patch *patch, const double c[4]);

/* The same coefficient as an EXPRESSION in the physical coordinates: `expr` is a C expression in the doubles x, y, z (and
   pi), e.g. "1.0 + x * x + 0.5 * sin(pi * z)".  The library emits a kernel for it, compiles it with hiprtc for the device
   of the patch, keeps the code object on disk under the hash of its source ($IGX_CACHE_DIR, default ~/.cache/igx) and
   evaluates it on the resident Gauss points from the geometry map -- nothing is sampled on the host.  *cache_hit (may be
   NULL) = 1 when the code object came from the cache.  Spline geometries only.  The analogue of the reference's run-time
   compiled assemblers and their source-hash module cache (pyiga/compile.py:58-73,120-132), for the one input the jet-form
   kernels cannot express themselves. */
int igx_patch_set_coeff_expr(igx_patch *patch, const char *expr, int *cache_hit);

/* A function given as a C expression in x, y, z (same grammar), evaluated at the RESIDENT Gauss points into the device array
   d_out (igx_patch_gauss_slab planes x G1 [x G2]) -- the input of igx_load_vector_d, without sampling the function on the
   host and uploading it (the reference samples f on the Gauss grid: pyiga/assemble.py:283-309).  parametric = 0: x, y, z are
   the physical coordinates (spline geometry needed); 1: the parametric coordinates of the Gauss points. */
int igx_patch_eval_expr_d(igx_patch *patch, const char *expr, int parametric, double *d_out, int *cache_hit);

/* Host only (no device, no patch): compile the coefficient kernel of `expr` for the architecture `arch` ("gfx950") into the
   cache, or find it there; path_out (may be NULL) receives the file name.  What igx_patch_set_coeff_expr does first. */
int igx_rtc_compile(const char *expr, const char *arch, char *path_out, int path_len, int *cache_hit);

/* Coefficients of IGX_FORM: coef[4*r + s] is P_rs on the FULL tensor Gauss grid (G0 x G1 x G2, C order, host
   pointer) or NULL for an absent (zero) coefficient; r = jet index of the test function v, s = of the trial
   function u.  Copied.  Replaces the previous form of the patch. */
int igx_patch_set_form(igx_patch *patch, const double *const coef[16]);
/* The same with coefficient arrays that already live on the device, each over the RESIDENT Gauss slab
   (igx_patch_gauss_slab planes x G1 [x G2], C order): no host staging of full-grid arrays.  A failed call of either
   variant leaves the previously set form untouched. */
int igx_patch_set_form_d(igx_patch *patch, const double *const d_coef[16]);
/* igx_patch_set_form_d with the table  scale * d_a + d_b  formed by one kernel straight into the copy the patch keeps (no staging
   array): the tables of an iterate-dependent form -- d_a the fixed part (uploaded once, e.g. the viscous form, scale the
   viscosity), d_b the part evaluated from the iterate.  A NULL on one side counts as zero, an entry NULL on
   both sides stays absent; d_a or d_b itself may be NULL (not both).  Each entry is rounded as the host sum is: the product, then
   the sum.  A failed call leaves the previously set form untouched. */
int igx_patch_set_form_sum_d(igx_patch *patch, const double *const d_a[16], double scale, const double *const d_b[16]);

/* The same table given as C expressions in the physical coordinates x, y, z (and pi; the grammar of
   igx_patch_set_coeff_expr): expr[4*r + s] or NULL.  The FIELD kernel of the form is generated with the expressions inside
   -- geometry map, Jacobian, coefficients and the transformation to the parametric jet coefficients in one pass over the
   resident Gauss points; the coefficients never exist as arrays -- compiled for the device with hiprtc and cached on disk
   under the hash of its source.  The reference generates the field loop of a form with its inputs fused in and caches the
   compiled module the same way (pyiga/codegen/cython.py:673-701 generate_precomp, :325-387; pyiga/compile.py:58-73,
   120-132); nothing is sampled on the host.  Needs a spline geometry.  (A geometry whose control lines exceed the LDS of a
   block takes a generated kernel that evaluates the coefficients into arrays first.)  The call compiles; the kernel runs
   with the next operation that needs the fields.  *cache_hit (may be NULL): 1 if the code object came from the cache. */
int igx_patch_set_form_expr(igx_patch *patch, const char *const expr[16], int *cache_hit);
/* 1 if the patch's IGX_FORM is served by a generated field kernel (no coefficient arrays on the device), else 0. */
int igx_patch_form_generated(const igx_patch *patch);
/* Host only: compile the kernel that evaluates the n expressions into arrays for `arch` into the cache. */
int igx_rtc_compile_form(int n, const char *const *expr, const char *arch, char *path_out, int path_len, int *cache_hit);
/* Host only: compile the field kernel of the form expr[16] for a dim-dimensional geometry with ncomp components
   (ncomp = dim + 1: NURBS) for `arch` into the cache (what igx_patch_set_form_expr does). */
int igx_rtc_compile_form_fields(int dim, int ncomp, const char *const expr[16], const char *arch, char *path_out, int path_len, int *cache_hit);

/* Parametric jet form for IGX_FORM -- forms with second derivatives (hess, Dx(.., times=2)) and parametric derivatives
   (parametric=True) of the reference (pyiga/vform.py:592-625 physical Hessians from parametric ones, :1518-1586 Dx / grad /
   hess), which its code generator differentiates symbolically (pyiga/vform.py:540-607) and compiles per form:

       a(u, v) = sum_k  integral over the parameter domain of  c_k(xi) * D^(mv_k) v(xi) * D^(mu_k) u(xi)  d xi

   with n <= 16 terms per call.  masks[2k] = mv_k, masks[2k+1] = mu_k: bit a set = on GRID axis a the function enters with
   slot 1 of that axis' basis table, else with slot 0.  The slots hold the derivative orders set by igx_patch_set_basis_orders
   ((0, 1) = value / first derivative by default), so one call covers the terms whose derivative orders fit one choice of two
   orders per axis; the host (pyiga_amd/pforms.py) splits a form into such passes and adds the results.  coef[k]: host array
   over the FULL Gauss grid, WITHOUT the Gauss weights (the geometry factors -- |det J|, J^-1, the Hessian of the geometry map --
   are the caller's: they are part of c_k).  Copied; replaces the previous form of the patch (either kind). */
int igx_patch_set_pform(igx_patch *patch, int n, const int *masks, const double *const *coef);
/* Derivative orders (0 <= slot0[a] < slot1[a] <= 2, one pair per axis) held by the two slots of the basis tables.  With
   anything but (0, 1) on every axis the patch assembles a parametric jet form only (every other call fails with
   IGX_ERR_ARG until the default is restored). */
int igx_patch_set_basis_orders(igx_patch *patch, const int *slot0, const int *slot1);

/* Gauss grid and weights of axis k (host copies; length ngauss[k]) */
int igx_patch_gauss(const igx_patch *patch, int axis, double *nodes, double *weights);

/* Resident Gauss planes of axis 0: a row slab keeps only the planes its rows touch, [*g0_lo, *g0_lo + *g0_n).
   Device-side inputs (igx_load_vector_d) are laid out on this slab. */
int igx_patch_gauss_slab(const igx_patch *patch, int64_t *g0_lo, int64_t *g0_n);

/* IGX_PATH_* bits of the last sum-factorised assembly of this patch (0: none yet / entry-wise) */
int igx_patch_last_path(const igx_patch *patch);

/* Canonical CSR pattern of the owned rows.  indptr has (row_hi-row_lo+1) entries, LOCAL
   (indptr[0] = 0); indices has nnz entries (global column ids).  Either may be NULL.
   The pattern is also kept on the device. */
int igx_pattern(igx_patch *patch, int32_t *indptr, int32_t *indices);

/* Assemble all CSR values of the owned rows into device memory (symmetric: lower triangle
   computed, strict lower part mirrored -> exactly symmetric, as assemble_entries(symmetric=True);
   IGX_CONVDIFF is non-symmetric: every entry is computed, as assemble_entries(symmetric=False)).
   If data_out != NULL the nnz values are also copied to the host buffer. */
int igx_assemble(igx_patch *patch, int kind, int algo, double *data_out);
int igx_last_timing(const igx_patch *patch, igx_timing *t);

/* Device pointers of the most recent results (valid until the patch is destroyed) */
const double  *igx_d_csr_data(const igx_patch *patch);
const int32_t *igx_d_csr_indices(const igx_patch *patch);
const int32_t *igx_d_csr_indptr(const igx_patch *patch);

/* Low-rank (adaptive cross approximation) assembly of the mass / stiffness matrix of a whole patch: the algorithm of
   pyiga/fastasm.cc:294-494,701-760 (fast_assemble_2d/3d, reached from mass_fast/stiffness_fast, pyiga/assemble.py:1063-1101)
   on the host, pulling whole rows / columns / fibres of the reordered matrix from the device with batched entry requests
   instead of one callback per entry.  data_out: nnz values in the canonical CSR order of igx_pattern (approximate to
   `tol`).  rank_out: crosses added; entries_out: entries actually evaluated.  Defaults of the reference: tol 1e-10,
   maxiter 100, skipcount 3, tolcount 3; verbose 0..2 prints the reference's progress lines to stdout. */
int igx_fast_assemble(igx_patch *patch, int kind, double tol, int maxiter, int skipcount, int tolcount, int verbose,
                      double *data_out, int *rank_out, long long *entries_out);
/* Request granularity of igx_fast_assemble.  A request is one launch: the index pairs of whole lines / slices of the
   reordered tensor are generated on the device from resident per-axis tables (nothing is uploaded), only the values come
   back.  A slice (3D) or the whole matrix (2D) with at most `max_entries` entries is fetched exactly in ONE request instead
   of being approximated line by line (on this hardware a launch costs as much as ~2000 entries); 0 = always line by line (the
   reference's access pattern).  Default 65536. */
int igx_patch_set_aca_batch(igx_patch *patch, long long max_entries);
/* Counters of the last igx_fast_assemble of the patch: batched requests (launches), entries evaluated, crosses. */
int igx_fast_assemble_stats(const igx_patch *patch, long long *requests, long long *entries, int *rank);

/* multi_entries: ij is M x 2 (row, col) of ravelled dof indices; out[k] = 0.0 for pairs whose
   supports do not intersect.  Works for any pair, inside or outside the owned slab provided the
   fields of the pair's Gauss points are resident (always true for a full patch). */
int igx_entries(igx_patch *patch, int kind, const size_t *ij, size_t M, double *out);

/* The same with the index pairs and the results in device memory (no copies; pyiga/genericasm.pxi:722-758). */
int igx_entries_d(igx_patch *patch, int kind, const size_t *d_ij, size_t M, double *d_out);

/* Device buffers that stay resident between calls (function values, index pairs, results): plain hipMalloc'ed memory on the
   context's GPU; uploads / downloads are synchronous on the context's stream. */
void *igx_dev_alloc(igx_ctx *ctx, size_t bytes);                               /* NULL on failure */
void  igx_dev_free(igx_ctx *ctx, void *d_ptr);
int   igx_dev_upload(igx_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int   igx_dev_download(igx_ctx *ctx, void *dst, const void *d_src, size_t bytes);

/* Load vector of the owned rows: out[i] = sum over the Gauss grid of  B_i * f * gw0*gw1*gw2*|det J|
   (inner_products(kvs, f, geo=geo), L2FunctionalAssembler*.assemble_vector()).  fvals: the function on the
   FULL tensor Gauss grid (G0 x G1 [x G2], C order, host), i.e. utils.grid_eval(f, gaussgrid) or
   grid_eval_transformed(f, gaussgrid, geo); out: (row0_hi-row0_lo) x N1 [x N2] doubles (host). */
int igx_load_vector(igx_patch *patch, const double *fvals, double *out);

/* The same with the function values of the RESIDENT Gauss slab (G0_local x G1 [x G2], C order) and the result in device
   memory: no transfer, workspace owned by the patch (pyiga/assemble.py:288-340 with f already sampled). */
int igx_load_vector_d(igx_patch *patch, const double *d_fvals, double *d_out);

/* Linear functional in the first-order jet of v:  out[i] = integral of  sum_r F_r(x) D_r v_i  dx  (D_0 = id, D_1.. =
   physical derivatives).  coef[r]: F_r on the FULL tensor Gauss grid (host) or NULL.  Arity-1 form strings such as
   'inner(b, grad(v)) * dx' (pyiga/assemble.py:837-897).  Replaces the IGX_FORM coefficients of the patch. */
int igx_load_vector_jet(igx_patch *patch, const double *const coef[4], double *out);
/* The same functional with its coefficients given as C expressions in the physical coordinates x, y, z (expr[r] or NULL; the
   grammar and the run-time compilation of igx_patch_set_form_expr): nothing is sampled on the host. */
int igx_load_vector_jet_expr(igx_patch *patch, const char *const expr[4], double *out, int *cache_hit);
/* Load vector of a scalar function given as ONE C expression in x, y, z -- the physical coordinates, or with parametric != 0
   the parametric ones (pyiga/assemble.py:288-340, inner_products with f_physical = True / False).  3D patches that the fused
   contraction kernel serves (equal degrees 1..5 on the last two axes, at most 640 Gauss points per line): a generated variant
   of that kernel evaluates the function at the points of its grid line -- the function values never exist as an array; the
   weight field of the patch is computed once and kept.  Anything else: IGX_ERR_UNSUPPORTED (igx_patch_eval_expr_d +
   igx_load_vector_d serve it with one full-grid array).  A function of the physical coordinates needs a spline geometry. */
int igx_load_vector_expr(igx_patch *patch, const char *expr, int parametric, double *out, int *cache_hit);
/* Host only: compile that kernel (P = degree + 1 of the last two axes, npass = max(2, ceil(dofs of the last axis / 64)) <= 4). */
int igx_rtc_compile_load_vector(int P, int npass, int parametric, const char *expr, const char *arch, char *path_out, int path_len, int *cache_hit);

/* --- fields evaluated on the device as inputs of form coefficients (Newton's method) ------------------
   A spline of the patch's OWN space (same knot vectors and degrees), given by its dofs in device memory (N0 x N1 [x N2]
   doubles, C order), at the resident Gauss points.  d_out[0] receives the value; with want_grad != 0, d_out[1 .. dim] receive
   the PHYSICAL gradient in the jet order of the form tables (D_1 = d/dx, x belonging to the last grid axis).  Every output is a
   device array over the resident slab (igx_patch_gauss_slab planes x G1 [x G2], C order: the layout of igx_load_vector_d and
   igx_patch_set_form_d).  One pass over the dofs (pyiga/bspline.py:880-921, BSplineFunc.grid_eval / grid_jacobian, with the
   coefficients resident).  A row slab or a span box: IGX_ERR_UNSUPPORTED; a geometry given as Jacobian arrays serves
   want_grad = 0 only (IGX_ERR_UNSUPPORTED otherwise).  igx_last_timing: total_ms = the kernels, algo_used = 4. */
int igx_patch_eval_spline_d(igx_patch *patch, const double *d_coeffs, int want_grad, double *const d_out[4]);
/* nc = 2 or 3 (else IGX_ERR_ARG) splines of the patch's own space in one pass: their dofs component-major in one device vector
   (nc x N0 x N1 [x N2] doubles: the velocity part of a saddle-point solver's vector).  d_out[c], c < nc, receives the value of
   component c; with want_grad != 0, d_out[nc + c * dim + r], r < dim, receives its physical partial r in the jet order above:
   nc * (1 + dim) arrays, each over the resident slab.  The geometry Jacobian is evaluated and inverted once per point for all
   components.  Component c has the bits of igx_patch_eval_spline_d on the dofs of component c, value and gradient.  Refusals as
   igx_patch_eval_spline_d's; the line buffers hold nc times as much, so the longest last axis that fits is shorter. */
int igx_patch_eval_vspline_d(igx_patch *patch, int nc, const double *d_coeffs, int want_grad, double *const d_out[12]);
/* igx_patch_set_form_expr's coefficient kernel with m <= 16 further doubles f0 .. f{m-1} in scope, loaded from the device arrays
   d_in[0 .. m) at the thread's resident Gauss point:  d_out[k * npts + i] = expr_k(x, y, z, pi, f0, ..) for the n expressions
   (npts = resident points).  Same grammar, same refusals and the same on-disk cache (m is part of the generated source).  With a
   geometry given as Jacobian arrays x, y, z are the parametric coordinates.  The arrays of igx_patch_eval_spline_d go in, the
   result goes to igx_patch_set_form_d / igx_load_vector_jet_d (pyiga/codegen/cython.py:673-701 evaluates updatable inputs in
   the field loop of the generated assembler).  igx_last_timing: total_ms = the kernel, algo_used = 5. */
int igx_patch_eval_exprs_inputs_d(igx_patch *patch, int n, const char *const *expr, int m, const double *const *d_in, double *d_out, int *cache_hit);
/* Host only: compile that kernel for `arch` (as igx_rtc_compile_form). */
int igx_rtc_compile_exprs_inputs(int n, const char *const *expr, int m, const char *arch, char *path_out, int path_len, int *cache_hit);
/* igx_load_vector_jet with the coefficients F_r on the RESIDENT Gauss slab in device memory (d_coef[r] or NULL) and the result
   (row0_hi-row0_lo) x N1 [x N2] doubles left in device memory.  Replaces the IGX_FORM coefficients of the patch. */
int igx_load_vector_jet_d(igx_patch *patch, const double *const d_coef[4], double *d_out);

/* --- integrals and error norms over a whole patch -----------------------------------------------------
   Every array is a device array over the resident Gauss points in the layout of igx_patch_eval_spline_d.  Total and per-element
   sums are formed in a fixed order without atomics: two calls with the same inputs return the same bits.  A row slab or a span
   box: IGX_ERR_UNSUPPORTED.  igx_last_timing: total_ms = the kernels, algo_used = 6.

   out[k] = sum over the patch of W f_k, W = gw |det J|, for 1 <= nf <= 4 arrays; d_elem: NULL or [nf][nelem] per-element sums,
   elements in span order (s0, s1[, s2]) row-major.  Replaces pyiga/assemble.py:658-697 (integrate) for one patch. */
int igx_patch_quad_sums_d(igx_patch *patch, int nf, const double *const *d_f, double *d_elem, double *out);
/* u_h: the spline of the patch's own space with the DEVICE dof vector d_coeffs.  d_exact (or NULL: all absent): d_exact[0] the
   exact values at the resident Gauss points or NULL; d_exact[1..dim]: the exact physical gradient in jet order (d/dx first, x the
   last grid axis) or NULL; all or none of the gradient arrays.  An absent array is zero.  out[0] = sum W (u_h - g)^2; with
   want_grad out[1] = sum W |grad u_h - grad g|^2 (a spline geometry: a geometry given as Jacobian arrays serves want_grad = 0
   only).  d_elem: NULL or [1 + want_grad][nelem]. */
int igx_patch_error_sums_d(igx_patch *patch, const double *d_coeffs, int want_grad, const double *const d_exact[4],
                           double *d_elem, double out[2]);
/* Element residual sums of u_h (as above) for the Poisson problem -Lap u = f:  out[0] = sum W (f + Lap u_h)^2, Lap the PHYSICAL
   Laplacian (second derivatives of u_h and of the geometry map at the Gauss points), out[1] = sum W.  d_f: the right-hand side at
   the resident Gauss points or NULL (= 0).  d_elem: NULL or [2][nelem] with the same two sums per element.  A geometry given as
   Jacobian arrays, a row slab or a span box: IGX_ERR_UNSUPPORTED, before anything is launched; a last axis whose line buffers
   ((3 in 2D, 6 in 3D) * ndofs + 2 * ngauss doubles) exceed 64 KB: IGX_ERR_UNSUPPORTED.  Any space is taken: where u_h is not C^1
   the sums are those of the element interiors (no jump terms). */
int igx_patch_residual_sums_d(igx_patch *patch, const double *d_coeffs, const double *d_f, double *d_elem, double out[2]);

/* Precomputed fields (W or upper triangle of B) of the owned Gauss slab: out has shape
   (F, G0_local, G1[, G2]) (structure-of-arrays).  For tests of precompute_fields. */
int igx_fields(igx_patch *patch, int kind, double *out, int64_t *shape4);

/* Mass / stiffness matrix of a 3D patch whose geometry is SEPARABLE along axis 0 -- G(xi0, xi1, xi2) = (g(xi1, xi2), z(xi0)),
   an extruded cross-section -- as the sum of Kronecker products
       mass:  M0 (x) M2D            stiffness:  M0 (x) K2D + K0 (x) M2D
   patch2: the 2D patch of the cross-section (axes 1, 2 of patch3: same knot vectors and the SAME number of Gauss points
   per span; the map g); m0, k0 (host, [ndofs0][2 p0 + 1], row i0, column jlo(i0) + k, zeros where no column): the 1D matrices
   int phi_i phi_j |z'| and int phi_i' phi_j' / |z'| on the Gauss rule of axis 0 of patch3 (k0 unused for the mass form).
   The library assembles the 2D matrices on patch2 and expands them into the canonical CSR values of the owned rows of
   patch3 (device-resident like igx_assemble; data_out as there, may be NULL).  The caller establishes separability (the
   Python front-end inspects the control net: geometry.split_axis0).  What the reference does for geo = None with 1D
   matrices (pyiga/assemble.py:125-190,236-282), extended to separable geometry maps. */
int igx_assemble_kron3(igx_patch *patch3, igx_patch *patch2, int kind, const double *m0, const double *k0, double *data_out);

/* --- boundary terms (Robin, impedance): A[bd, bd] += R on the device ----------------------------------
   Adds the matrix of a boundary integral over the side (axis, side) of the patch -- side 0: the dofs with i_axis = 0, side 1:
   those with i_axis = N_axis - 1 -- to the values the patch holds on the device.  The face space is the tensor product of the
   patch's other axes in their order; face entry (It, Jt) lands on volume entry (I, J), I and J being It and Jt with the side's
   index inserted at `axis`.  Every target position is arithmetic on the per-axis tables (no index arrays, no search); the add
   is a plain read-add-write (no atomics: within one face no two entries share a position), and successive calls run in stream
   order, so where two faces meet the value is ((a + r_1) + r_2) in the order of the calls.
   `face`: the (d-1)-dimensional patch of the face space holding its values on the device (igx_assemble(face, kind, algo, NULL));
   a 3D volume takes a 2D face patch.  The _host variant takes the nvals values of the face matrix in the canonical CSR order of
   the face space (rows of the face dofs, per row the columns jlo .. jhi of every face axis) and serves the 1D faces of 2D
   patches and any face matrix formed on the host.
   IGX_ERR_ARG: the patch holds no values (values_kind < 0), axis or side out of range, a face whose degrees, dof counts or
   per-axis column ranges differ from those of the patch's other axes, a wrong nvals.  IGX_ERR_UNSUPPORTED: a row slab or span
   box (either patch).  The kind of the values (values_kind) is unchanged, so igx_solver_create* and igx_solver_take_values accept
   them afterwards; a solver that ALREADY reads the patch's values must be told with igx_solver_values_changed.
   <- A[bd_dofs[:, None], bd_dofs] += R  on the host matrix */
int igx_patch_add_face(igx_patch *patch, int axis, int side, const igx_patch *face);
int igx_patch_add_face_host(igx_patch *patch, int axis, int side, const double *vals, int64_t nvals);

/* Opt-in buffer placement (environment IGX_PLACEMENT_TRIES=n at igx_patch_create, 3D symmetric forms): the first
   igx_assemble allocates up to n candidate buffers for the CSR values, times the mirror pass of the patch on each and keeps
   the fastest (the pass follows where the driver put the buffer physically: +-10 % between allocations, stable over the life
   of a buffer).  Reports how many candidates were timed (0: the search did not run) and the device time of the pass on the
   kept and on the slowest one.  (No counterpart in the reference.) */
int igx_patch_placement(const igx_patch *patch, int *tried, float *best_ms, float *worst_ms);

/* Planning query, host arithmetic only (no device, no patch): 1 if the fused sweep + contraction stage and the mirror pass
   may address a patch of these sizes with their 32-bit buffer offsets, 0 if the library takes the stage kernels with 64-bit
   addressing instead.  c0max = 2 p0 + 1 columns of axis 0 per row (1 in 2D), S_mid / S_last = number of 1D index pairs
   (i, j) of the mid / last axis, G_mid / G_last = their Gauss points.  The limits: a row block of one outer row
   (c0max * S_mid * S_last values) and one slice of the sweep intermediate (G_mid * G_last values) below 2^31 bytes.
   (No counterpart in the reference: its index type is size_t throughout, pyiga/assemble_tools_cy.pyx:44-49.) */
int igx_fused_stage_fits(int64_t c0max, int64_t S_mid, int64_t S_last, int64_t G_mid, int64_t G_last);

/* Planning queries of the same stage, host arithmetic only (no device, no patch; no counterpart in the reference).
   igx_fused_rows_per_tile: rows of the last axis a block of the stage takes for P = degree + 1 (2 .. 6) of the swept and the
   last axis, the slot set `mask` of the form (bit 4 y + t1: an input array enters the sweep with last-axis type y and
   mid-axis type t1; 0x0001 mass, 0x135F the full first-order set, 0x1248 2D stiffness) and na = 1 or 2 arrays per slot; -1
   where no kernel is compiled for the arguments.  The last axis of N dofs is cut into ceil(N / rows) tiles of equal height.
   igx_fused_chunk_plan: how a launch of npairs * ntiles blocks cuts the mid_rows rows of the swept axis on a chip that holds
   `slots` blocks at a time: out = { rows per chunk, chunks, main_blocks, tail_k, tail_rows }.  With tail_k = 0 every block
   walks one of the chunks; with tail_k > 0 (then chunks = 1) the first main_blocks blocks walk the whole axis and each of
   the others one of tail_k chunks of tail_rows rows, the last one clipped.  IGX_ERR_ARG for arguments out of range. */
int igx_fused_rows_per_tile(int P, int mask, int na);
int igx_fused_chunk_plan(int npairs, int ntiles, int mid_rows, int64_t slots, int P, int out[5]);

/* Planning queries of a patch, host arithmetic only: nothing is launched (no counterpart in the reference).  Each returns what
   the launcher itself decides with -- the query and the launch call one function.
   igx_patch_fields_plan: the kernel that forms the quadrature fields of `kind` from the geometry map.
     out = { line-wise (1) or point-wise (0), lines per block, bytes of LDS of a block, components of the control net incl. the
     NURBS weight (0: Jacobian array) }; lines per block and bytes are 0 for the point-wise kernel (Jacobian arrays, span boxes,
     line coefficients above 64 KiB).  (A form given as expressions has a generated field kernel of its own, not described here.)
   igx_patch_single2d_plan: the tile of the single-launch 2D mass / stiffness kernel, for the resident rows or (whole_patch != 0)
     as if the patch were whole.  out = { supported, wanted (the assembly would take this kernel: small patches, or IGX_PATH=single),
     rows per tile along axis 0, along axis 1, Gauss planes of axis 0 in LDS, window points of axis 1, geometry control columns
     of axis 1 in LDS, bytes of LDS, blocks of the launch }; everything after `wanted` is 0 where the kernel does not support the
     patch or no tile fits LDS.
   IGX_ERR_ARG: null argument, unknown kind. */
int igx_patch_fields_plan(const igx_patch *patch, int kind, int64_t out[4]);
int igx_patch_single2d_plan(const igx_patch *patch, int kind, int whole_patch, int64_t out[9]);

/* --- multipatch: sum_p X_p A_p X_p^T on the device (pyiga/assemble.py:1103-1389) -------------------------------------------
   X_p is the 0/1 matrix of the local-to-global map l2g[p] (Multipatch.patch_to_global_idx, pyiga/assemble.py:1276-1293).  The
   handle does NOT own the patches: they are read by the calls that take them and may be destroyed afterwards. */
typedef struct {
    int32_t npatches;
    int32_t injective;         /* 1 if every map l2g[p] is injective (else the sums are formed with atomics: correct to rounding) */
    int64_t nrows;             /* global dofs */
    int64_t nnz;               /* entries of the global pattern */
    int64_t entries[4];        /* local entries over all patches by scatter class: direct store, store through a position,
                                  read-add-write, atomic add */
    int64_t zero_from;         /* igx_multipatch_zero clears the values from this position on */
} igx_multipatch_info;

/* Builds the canonical CSR pattern (sorted, unique int32 columns per row) of sum_p X_p S_p X_p^T from the device pattern S_p
   of every patch (igx_pattern; built here if missing) and l2g[p] (host, nrows_total of patch p entries in [0, nglobal)),
   entirely on the device, and the scatter plan of every patch.  Entries whose values sum to 0 stay in the pattern (scipy
   would drop them).  Whole patches only (no row slab, no span box).  A global nnz of 2^31 or more: IGX_ERR_UNSUPPORTED
   (igx_last_error).  NULL on failure.  <- Multipatch.finalize + the pattern of A += X @ A_p @ X.T (pyiga/assemble.py:1264-1270,
   1340-1370) */
igx_multipatch *igx_multipatch_create(igx_ctx *ctx, int npatches, igx_patch *const *patches, const int32_t *const *l2g, int64_t nglobal);
void igx_multipatch_destroy(igx_multipatch *mp);
int  igx_multipatch_get_info(const igx_multipatch *mp, igx_multipatch_info *info);
/* Global pattern to host: indptr has nrows + 1 entries, indices nnz.  Either may be NULL.  <- (A.indptr, A.indices) */
int  igx_multipatch_pattern(const igx_multipatch *mp, int32_t *indptr, int32_t *indices);
/* Start a new sum: A = 0, b = 0 (the reference's  A = csr_matrix((n, n)); b = zeros(n)).  Rows that one local row reaches are
   overwritten by its scatter; only the rows of interface dofs are cleared. */
int  igx_multipatch_zero(igx_multipatch *mp);
/* A += X_p A_p X_p^T with the values A_p that `src` holds on the device after igx_assemble(src, ..., data_out = NULL) -- nothing
   goes through the host.  `src` must have patch p's shape and nnz (IGX_ERR_ARG otherwise).  One pass on the context's stream,
   read-add-write in the rows of interface dofs: calls in patch order sum as ((0 + a_0) + a_1) + ..., bit for bit the
   reference's order.  Returns when the pass is done (`src` may then be destroyed).  <- A += X @ A_p @ X.T */
int  igx_multipatch_scatter_patch(igx_multipatch *mp, int p, const igx_patch *src);
/* The same with the nnz values of patch p in its canonical CSR order given on the host. */
int  igx_multipatch_scatter_host(igx_multipatch *mp, int p, const double *vals);
/* b += X_p b_p, b_p host (nrows_total of patch p values).  <- b += X @ b_p */
int  igx_multipatch_scatter_vector(igx_multipatch *mp, int p, const double *b);
/* Global values (nnz, in the order of igx_multipatch_pattern) and vector (nrows) to host.  Either may be NULL. */
int  igx_multipatch_download(const igx_multipatch *mp, double *vals, double *vec);
/* The nnz values of the current sums, in the order of igx_multipatch_pattern, copied device to device into the caller's buffer
   (nnz doubles of the same context): what a second matrix over the same pattern is made of (igx_solver_set_mass_d). */
int  igx_multipatch_values_d(const igx_multipatch *mp, double *d_out);
/* igx_patch_add_face[_host] on the global sums: the face matrix of side (axis, side) of patch p is added at the positions its
   volume entries were scattered to (the patch's row plan: position + delta for rows stored directly, the position array
   otherwise).  Call it after the scatters of the current sum: read-add-write, in stream order (atomic adds only where a map
   l2g[p] is not injective).  Before patch p was scattered into the current sum (since igx_multipatch_zero): IGX_ERR_ARG, because
   the scatter's plain stores would overwrite the add.  Other errors as igx_patch_add_face.  Add before igx_solver_create_multipatch: a
   solver made earlier has gathered its Jacobi diagonal from the older values. */
int  igx_multipatch_add_face(igx_multipatch *mp, int p, int axis, int side, const igx_patch *face);
int  igx_multipatch_add_face_host(igx_multipatch *mp, int p, int axis, int side, const double *vals, int64_t nvals);

/* --- Dirichlet problems of one patch on the device: preconditioned CG (pyiga/assemble.py:571-652, pyiga/solvers.py:17-42) ----
   The solver reads the CSR values that the patch holds on the device after an assembly with data_out = NULL, in the patch's own
   structured layout (no index arrays).  Dirichlet dofs are handled with a dof mask: every vector is full-length with zeros at the
   fixed dofs, and the restricted matrix R A R^T never exists.  The handle does NOT own the patch: the patch must outlive it. */
typedef struct igx_solver igx_solver;
enum { IGX_PRECOND_NONE = 0, IGX_PRECOND_JACOBI = 1, IGX_PRECOND_KRON = 2,
       IGX_PRECOND_SCHWARZ = 3,     /* multipatch solvers only: set up by igx_solver_set_schwarz */
       IGX_PRECOND_MG = 4 };        /* multipatch solvers, CG only: one V-cycle of the hierarchy set up by igx_solver_set_[block_]mg_* */
/* how the per-axis eigenvalues lam_k form the diagonal D of a Kronecker preconditioner  (x)U_k . D^-1 . (x)U_k^T */
enum { IGX_KRON_SUM = 1,       /* D = sum_k 1 (x) .. (x) lam_k (x) .. (x) 1: fast diagonalization of sum_k K_k (x) M_rest (Sangalli-Tani) */
       IGX_KRON_PRODUCT = 2 }; /* D = (x)_k lam_k: with U_k, lam_k the eigenpairs of M_k this is (x) M_k^-1 */

typedef struct {
    int32_t iterations;        /* CG iterations done */
    int32_t converged;         /* 1 if ||r|| <= tol * ||R (b - A ext(g))|| was reached */
    double relres;             /* final ||r|| / ||R (b - A ext(g))|| */
    int64_t n_free;            /* free dofs */
    float spmv_ms, precond_ms, vector_ms;   /* device time summed over the iterations (solve with timed != 0, else 0) */
    float total_ms;            /* device time of the whole solve, transfers included */
} igx_solve_info;

/* A solver for the matrix of `kind` (IGX_MASS or IGX_STIFFNESS only -- CG needs a symmetric positive definite matrix; any other
   kind: IGX_ERR_UNSUPPORTED) that the patch holds on the device now (else IGX_ERR_ARG).  fixed[0..nfixed): the eliminated dofs
   (ravelled indices; the order of the values given to the solve).  Whole patches only: a row slab or a span box is
   IGX_ERR_UNSUPPORTED.  *out receives the handle (NULL on failure). */
int  igx_solver_create(igx_patch *patch, int kind, const int64_t *fixed, int64_t nfixed, igx_solver **out);
/* A solver for the global sum sum_p X_p A_p X_p^T that `mp` holds now (after igx_multipatch_zero and the scatters), in its
   CSR pattern on the device.  fixed[0..nfixed): eliminated global dofs (Multipatch.compute_dirichlet_bcs).  The matrix must be
   symmetric positive definite on the free dofs (CG).  The handle does NOT own `mp`: the multipatch must outlive it.  Once
   igx_multipatch_zero has restarted the sums, every call that reads them returns IGX_ERR_ARG.  Preconditioners: NONE, JACOBI,
   SCHWARZ (igx_solver_set_schwarz); IGX_PRECOND_KRON: IGX_ERR_UNSUPPORTED.  The solve takes b = NULL: the multipatch's summed
   vector on the device. */
int  igx_solver_create_multipatch(igx_multipatch *mp, const int64_t *fixed, int64_t nfixed, igx_solver **out);
void igx_solver_destroy(igx_solver *solver);
/* Preconditioner of the following solves.  IGX_PRECOND_NONE; IGX_PRECOND_JACOBI: the diagonal, gathered from the device values;
   IGX_PRECOND_KRON: (x)U_k . D^-1 . (x)U_k^T on the free box box_lo[k] <= i_k < box_hi[k], which must be exactly the free dofs.
   U[k] (host, n_k x n_k row-major, n_k = box_hi[k] - box_lo[k]) and lam[k] (host, n_k) per axis, lam_mode IGX_KRON_*.  The
   other arguments may be NULL for NONE and JACOBI. */
int igx_solver_set_precond(igx_solver *solver, int precond, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                           const double *const *lam, int lam_mode);
/* Additive Schwarz preconditioner of a multipatch solver (and selects it; afterwards igx_solver_set_precond(IGX_PRECOND_SCHWARZ)
   selects it again):  z = sum_p X_p M_p B_p M_p X_p^T r,  M_p the mask of the free dofs, B_p = (x)U_k . D^-1 . (x)U_k^T the
   fast-diagonalization inverse of patch p on the box box_lo[p*3+k] <= i_k < box_hi[p*3+k] of its local dofs (a patch with an
   empty box takes no part).  U[p*3+k] (host, n_k x n_k row-major) and lam[p*3+k] (host, n_k) per patch and axis (axes beyond
   the patch's dimension are not read), lam_mode IGX_KRON_*.  Patch solvers, or a multipatch whose maps are not all injective:
   IGX_ERR_UNSUPPORTED. */
int igx_solver_set_schwarz(igx_solver *solver, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                           const double *const *lam, int lam_mode);
/* --- Newton's method on a scalar patch solver (igx_solver_create_general): iterate, residual and Jacobian
   stay in device memory; any other solver: IGX_ERR_UNSUPPORTED -----------------------------------------------------------------
   The caller knows the matrix of the solver's kind to be symmetric positive definite (a traced coefficient table that is
   symmetric): igx_solver_set_method(IGX_METHOD_CG) is accepted from now on. */
int igx_solver_declare_symmetric(igx_solver *solver);
/* The patch's values of the solver's OWN kind were assembled again (a new Jacobian): the staleness check of the solves is passed
   as before, and the diagonal of the Jacobi preconditioner, if that is the one selected, is gathered again.  Values of another
   kind, or none: IGX_ERR_ARG as in igx_solver_solve. */
int igx_solver_values_changed(igx_solver *solver);
/* *norm = || R v ||_2 of the full-length device vector v, R the restriction to the free dofs.  One double comes back. */
int igx_solver_masked_norm_d(igx_solver *solver, const double *d_v, double *norm);
/* One Newton update  x -= R^T (R J R^T)^-1 R F  with the full-length device vectors d_F and d_x and the matrix J the patch holds:
   the linear solve starts from zero with zero fixed values, to ||r|| <= tol ||R F|| (the solver's method and preconditioner), and
   the fixed entries of d_x are left as they are (pyiga/solvers.py:335-361, the step of newton()). */
int igx_solver_newton_update_d(igx_solver *solver, const double *d_F, double *d_x, double tol, int maxiter, int check_every,
                               igx_solve_info *info);
/* --- Geometric multigrid over a hierarchy of multipatch solvers (IGX_PRECOND_MG) -----------------------
   A hierarchy is a chain of multipatch solvers, the finest first, each over the sums of the same problem on a coarser, nested
   space with the same sides fixed.  Every solver of the chain gets a smoother (all but the coarsest) and either the next coarser
   solver or the dense inverse of its matrix.  No handle owns another: all of them, and their multipatches, must outlive the
   calls that walk the chain; destroying a solver unlinks it from its neighbours (the finer one loses IGX_PRECOND_MG), and a level
   whose multipatch restarted its sums makes every call that applies the hierarchy return IGX_ERR_ARG.  `level` below counts
   from the solver given (0) down the chain.

   First-fit colouring of the graph of a CSR pattern (n rows; a symmetric pattern is assumed) restricted to the rows with
   free_mask[i] != 0 (NULL: all rows): the rows are visited in ascending order and take the smallest colour none of their coloured
   neighbours has.  colour[i] (n entries) is -1 on the other rows; *ncolours (may be NULL) the number of colours.  Host code:
   needs no context and no device. */
int igx_csr_colouring(int64_t n, const int32_t *indptr, const int32_t *indices, const uint8_t *free_mask, int32_t *colour,
                      int32_t *ncolours);
/* The Gauss-Seidel smoother of a multipatch solver: colour[i] (host, all dofs; read on the free dofs) such that no two coupled
   free dofs share a colour (checked against the pattern: IGX_ERR_ARG names the first pair).  A forward sweep relaxes the colours
   in ascending order, a backward sweep in descending order, one launch per colour; a level of at most block_rows free dofs runs
   each sweep in a single launch of one block.  smooth_steps (1 .. 16): sweeps before and after the coarse correction. */
int igx_solver_set_mg_smoother(igx_solver *solver, const int32_t *colour, int smooth_steps, int64_t block_rows);
/* `coarse` becomes the next level of `solver`.  Both are multipatch solvers over the same number of patches with injective maps
   (else IGX_ERR_UNSUPPORTED).  P[p*3+k] (host, row-major, fine x coarse dofs of axis k of patch p; axes beyond the patch's dimension
   are not read): the 1D prolongation matrices, of which only the band of every row and column is kept.  mult (host, the fine
   solver's dofs): the number of patches every dof belongs to.  Prolongation: x_f = P x_c on the free dofs, P = W^-1 sum_p X_pf
   (P_0 (x) P_1 (x) P_2) X_pc^T, stored patch after patch; restriction: its transpose. */
int igx_solver_set_mg_coarse(igx_solver *solver, igx_solver *coarse, const double *const *P, const double *mult);
/* The coarsest level: inv (host, m x m row-major, m = free dofs of `solver` in ascending order) is applied as a dense product. */
int igx_solver_set_mg_inverse(igx_solver *solver, const double *inv, int64_t m);
typedef struct {
    int64_t nrows, nfree, nnz; /* dofs, free dofs and stored entries of the level's matrix */
    int32_t ncolours;          /* of the smoother (0: none) */
    int32_t one_block;         /* 1 if a sweep is a single launch of one block */
    int32_t smooth_steps;
    int32_t dense_inverse;     /* 1 if the level is solved with a dense inverse */
    int32_t has_coarse;        /* 1 if a coarser level is attached */
    int32_t reserved;
} igx_mg_info;
int igx_solver_mg_info(igx_solver *solver, int level, igx_mg_info *out);
/* The smoother's order of a level: rows (host, nfree) are the free dofs sorted by (colour, index), colour c at
   colour_offsets[c] .. colour_offsets[c + 1] (host, ncolours + 1). */
int igx_solver_mg_colours(igx_solver *solver, int level, int32_t *rows, int32_t *colour_offsets);
/* The pieces alone, on device vectors of all dofs of their level (fixed entries are ignored on input and 0 on output):
   one sweep in place on d_x with the right-hand side d_b, forward or backward (backward != 0); d_xf = P d_xc from level + 1 to
   level; d_rc = P^T d_rf from level to level + 1.  The two buffers of a call must differ. */
int igx_solver_mg_relax_d(igx_solver *solver, int level, int backward, const double *d_b, double *d_x);
int igx_solver_mg_prolong_d(igx_solver *solver, int level, const double *d_xc, double *d_xf);
int igx_solver_mg_restrict_d(igx_solver *solver, int level, const double *d_rf, double *d_rc);

/* Device time of the phases of one V-cycle d_z = B d_r (the mean of `reps` cycles; events between the phases): per level the
   sweeps, the residual (the CSR SpMV) and the transfers to and from the next level, the dense product of the coarsest level, the
   additions of the corrections, and the kernels one cycle launches (memsets not counted). */
#define IGX_MG_MAX_LEVELS 16
typedef struct {
    int32_t levels, launches;
    float total_ms, coarse_ms, vector_ms, reserved;
    float smooth_ms[IGX_MG_MAX_LEVELS], residual_ms[IGX_MG_MAX_LEVELS], transfer_ms[IGX_MG_MAX_LEVELS];
} igx_mg_profile;
int igx_solver_mg_profile_d(igx_solver *solver, const double *d_r, double *d_z, int reps, igx_mg_profile *out);

/* d_z = P d_r on the device with the current preconditioner P (full-length vectors; NONE: the free entries of d_r).  d_r and
   d_z must not overlap (d_z is cleared before d_r is read); the same buffer for both is refused with IGX_ERR_ARG. */
int igx_solver_precond_d(igx_solver *solver, const double *d_r, double *d_z);
/* d_y = R A R^T d_x on the device (full-length vectors; the fixed entries of d_x are ignored, those of d_y are 0). */
int igx_solver_spmv_d(igx_solver *solver, const double *d_x, double *d_y);
/* Solves  R A R^T x = R (b - A ext(g))  by CG and returns the full vector u = x + ext(g) (host, nrows_total).  b: host load
   vector (nrows_total); g: host values of the fixed dofs (in the order of `fixed`); x0: host initial guess (nrows_total, only
   its free entries are used) or NULL.  Stops when ||r|| <= tol * ||R (b - A ext(g))|| or after maxiter iterations; the residual
   norm is read back every check_every iterations (alpha and beta stay on the device).  timed != 0: events between the phases
   of every iteration (info->spmv_ms etc.).  The solve is deterministic: the same inputs give bit-identical u.  Refused
   (IGX_ERR_ARG) if the patch's values have been overwritten by an assembly of another kind since the solver was made.  A
   multipatch solver takes b = NULL: the right-hand side is then the multipatch's device vector. */
int igx_solver_solve(igx_solver *solver, const double *b, const double *g, const double *x0, double tol, int maxiter,
                     int check_every, int timed, double *u, igx_solve_info *info);

/* --- Non-symmetric Dirichlet problems: right-preconditioned BiCGStab (van der Vorst; the "Templates" variant that
   scipy.sparse.linalg.bicgstab runs).  r stays the true residual, so the stopping rule is CG's.  Two SpMVs and two applies of the
   preconditioner per iteration; its scalars stay on the device.  When rho = r^.r has cancelled to below eps^2 times the sum of
   the magnitudes of its terms, the iteration restarts with r^ = p = r.  The solve stops without converging (info->converged = 0)
   on a breakdown: rho vanishing again right after a restart, a step 1e-13 |alpha| ||v|| > ||r|| (r^.v vanished), t.t = 0 or
   omega = 0, or a non-finite scalar.  u is then the last finite iterate.  A solve that has stopped leaves x and r as they are, so
   check_every does not change u; info->iterations counts the iterations entered. */
enum { IGX_METHOD_CG = 0, IGX_METHOD_BICGSTAB = 1,
       IGX_METHOD_MINRES = 2 };      /* saddle-point solvers (igx_solver_create_saddle), and only they */
enum { IGX_BREAKDOWN_RHO = 1,        /* rho = r^.r vanished twice in a row (the restart with r^ = r did not help) */
       IGX_BREAKDOWN_ALPHA = 2,      /* r^.v vanished: the step alpha v would exceed 1e13 ||r|| */
       IGX_BREAKDOWN_OMEGA = 3,      /* t.t = 0 or omega = 0: the half step x + alpha p^ is kept */
       IGX_BREAKDOWN_NONFINITE = 4,  /* a scalar was not finite */
       IGX_BREAKDOWN_INDEFINITE_PRECOND = 5 };   /* MINRES: r.(P r) < 0, the preconditioner is not positive definite */
/* As igx_solver_create, for any kind the patch holds on the device (IGX_MASS, IGX_STIFFNESS, IGX_CONVDIFF, IGX_FORM; another
   value: IGX_ERR_ARG), with the same refusals (row slabs and span boxes, values not assembled or stale).  Starts in
   IGX_METHOD_BICGSTAB.  The patch's values must be the whole matrix of the form (a parametric jet form assembled in passes
   leaves only the last pass on the device). */
int  igx_solver_create_general(igx_patch *patch, int kind, const int64_t *fixed, int64_t nfixed, igx_solver **out);
/* The method of the following solves, on any solver.  IGX_METHOD_CG on a patch solver of a kind other than IGX_MASS /
   IGX_STIFFNESS: IGX_ERR_UNSUPPORTED.  IGX_METHOD_BICGSTAB allocates its four extra vectors once (a CG solver has none).
   IGX_METHOD_MINRES on a solver that is not a saddle-point solver, and any other method on one: IGX_ERR_UNSUPPORTED. */
int  igx_solver_set_method(igx_solver *solver, int method);
/* IGX_BREAKDOWN_* of the last solve, 0 if it did not break down (and for CG). */
int  igx_solver_last_breakdown(const igx_solver *solver);

/* --- Vector-valued forms (bfuns = [('u', nc), ('v', nc)]: elasticity, grad-div, ...): a block solver over the nc x nc scalar
   IGX_FORM blocks A_pq (test component p, trial component q), each in the patch's structured layout.  Vectors have nc * N entries,
   component-major (the reference's 'blocked' layout; N = nrows_total).  The block SpMV reads every block present once per product;
   an absent block is zero.  The solver owns its blocks and frees them in igx_solver_destroy; it does NOT own the patch, which
   must outlive the takes (re-assembling the patch afterwards leaves the solver as it is).  The other igx_solver_* calls work on
   it unchanged: IGX_PRECOND_JACOBI takes the diagonals of the diagonal blocks, IGX_PRECOND_KRON (box and factor arguments NULL)
   the block-diagonal preconditioner diag(P_0, .., P_{nc-1}) of the factors igx_solver_set_block_kron set per component.  A
   solve, an SpMV or the Jacobi set-up while a diagonal block is missing: IGX_ERR_ARG.
   A block solver of patch `patch` (whole patches only, as igx_solver_create) with ncomp = 2 or 3 components (else IGX_ERR_ARG);
   fixed[0..nfixed) index into the nc * N entries.  It starts in IGX_METHOD_CG if `symmetric`, else in IGX_METHOD_BICGSTAB;
   IGX_METHOD_CG on a solver made with symmetric = 0 is IGX_ERR_UNSUPPORTED.  No values are needed yet. */
int  igx_solver_create_block(igx_patch *patch, int ncomp, int symmetric, const int64_t *fixed, int64_t nfixed, igx_solver **out);
/* Moves the IGX_FORM values the patch holds now (igx_assemble(patch, IGX_FORM, algo, NULL)) into block (p, q): a hand-over of
   the device buffer, not a copy.  The patch then holds no values (its next assembly allocates anew).  p or q out of range, a
   block taken twice, or a patch without IGX_FORM values: IGX_ERR_ARG. */
int  igx_solver_take_block(igx_solver *solver, int p, int q);
/* Makes the IGX_FORM values the patch holds now the new block (p, q) of a live solver, whether the block is held already or
   absent so far (a nonlinear iteration: DESIGN.md section 33).  The old buffer goes back to the patch as its next values buffer,
   so that a replacement neither allocates nor frees; the patch then holds no values, as after igx_solver_take_block.  A selected
   IGX_PRECOND_JACOBI gathers the diagonal of a replaced diagonal block again; Kronecker factors, B, B^T, the masks and the
   projection state of a saddle-point solver are untouched.  Whether the new blocks fit the solver's method (CG: symmetric) is the
   caller's business.  Not a block solver of a patch, p or q out of range, or a patch without IGX_FORM values: IGX_ERR_ARG; a solver
   with an eigen-solver session: IGX_ERR_UNSUPPORTED. */
int  igx_solver_replace_block(igx_solver *solver, int p, int q);
/* hidden != 0: the products of a saddle-point solver leave the off-diagonal block (p, q) out, as if it were absent, until it is
   shown again (hidden = 0) or replaced; the solver keeps the buffer.  What a Picard step after a Newton step needs when the
   viscous form has no off-diagonal part: the Newton blocks must not enter the Picard residual, and nothing is freed.  Not a
   saddle-point solver: IGX_ERR_UNSUPPORTED; p == q or out of range: IGX_ERR_ARG. */
int  igx_solver_hide_block(igx_solver *solver, int p, int q, int hidden);
/* The fast-diagonalization inverse (x)U_k . D^-1 . (x)U_k^T of component `comp` on its free box box_lo[k] <= i_k < box_hi[k],
   which must be exactly the free dofs of that component (arguments as igx_solver_set_precond's, lam_mode IGX_KRON_*). */
int  igx_solver_set_block_kron(igx_solver *solver, int comp, const int32_t *box_lo, const int32_t *box_hi,
                               const double *const *U, const double *const *lam, int mode);

/* --- Vector-valued forms on a multipatch (elasticity on a multi-patch solid): a block solver over the nc x nc scalar blocks
   A_pq = sum_patch X A^{patch}_pq X^T, which all share the global CSR pattern of `mp`.  A global vector has
   nc * nrows entries, component-major; every component uses the scalar numbering and joins of the multipatch, and the mask of
   fixed dofs covers all nc * nrows entries.  One block SpMV per product reads every present block once.
   A block solver over the pattern of `mp` with ncomp = 2 or 3 components (else IGX_ERR_ARG); fixed[0..nfixed) are blocked
   global indices in [0, ncomp * nrows).  It starts in IGX_METHOD_CG if `symmetric`, else in IGX_METHOD_BICGSTAB; IGX_METHOD_CG
   on a solver made with symmetric = 0 is IGX_ERR_UNSUPPORTED.  The solver reads the pattern of `mp`, which must outlive it, but
   owns its value buffers: restarting the multipatch's sums afterwards leaves it as it is.  igx_solver_solve needs b (host,
   nc * nrows; NULL: IGX_ERR_ARG).  Preconditioners: NONE, JACOBI (the diagonals of the diagonal blocks), SCHWARZ once
   igx_solver_set_block_schwarz has set every component, MG once igx_solver_set_block_mg_* have completed a hierarchy (until then
   IGX_ERR_UNSUPPORTED); IGX_PRECOND_KRON and the eigen, parabolic, stepping and Newton calls: IGX_ERR_UNSUPPORTED. */
int  igx_solver_create_multipatch_block(igx_multipatch *mp, int ncomp, int symmetric, const int64_t *fixed, int64_t nfixed,
                                        igx_solver **out);
/* Copies the current sums of the multipatch (after igx_multipatch_zero and the scatters of EVERY patch: the interior rows are
   only ever overwritten, so a patch without values for this block scatters zeros) device to device into nnz doubles of the
   solver's own: block (p, q).  A block taken twice, p or q out of range, or sums restarted with nothing scattered since:
   IGX_ERR_ARG.  A block never taken is absent: zero, never read.  Peak memory: the present blocks plus the multipatch's own
   value array. */
int  igx_solver_take_multipatch_block(igx_solver *solver, int p, int q);
/* The nnz values of block (p, q) to the host, in the order of igx_multipatch_pattern (an absent block: IGX_ERR_ARG). */
int  igx_solver_download_multipatch_block(const igx_solver *solver, int p, int q, double *vals);
/* Per component, the additive Schwarz preconditioner of igx_solver_set_schwarz (same arguments) acting on the slice
   [comp * nrows, (comp + 1) * nrows) of the vectors with that component's mask.  Once every component is set,
   igx_solver_set_precond(IGX_PRECOND_SCHWARZ) selects diag(P_0, .., P_{nc-1}).  A multipatch whose maps are not all injective:
   IGX_ERR_UNSUPPORTED. */
int  igx_solver_set_block_schwarz(igx_solver *solver, int comp, const int32_t *box_lo, const int32_t *box_hi,
                                  const double *const *U, const double *const *lam, int lam_mode);
/* Geometric multigrid for multipatch block solvers: the hierarchy of igx_solver_set_mg_* over a chain of
   block solvers of the same problem, the lifetime rules included.  These three calls serve solvers of
   igx_solver_create_multipatch_block only (any other solver: IGX_ERR_UNSUPPORTED), and the scalar igx_solver_set_mg_* calls
   refuse them (IGX_ERR_UNSUPPORTED).  igx_solver_set_precond(IGX_PRECOND_MG) selects the V-cycle once the chain below the solver
   is complete; it needs IGX_METHOD_CG and a solver made with symmetric = 1 (else, and until then, IGX_ERR_UNSUPPORTED).
   igx_solver_mg_info, _colours, _relax_d, _prolong_d, _restrict_d and _profile_d serve such a hierarchy on vectors of
   ncomp * nrows entries: nrows and nfree of igx_mg_info count blocked dofs, nnz sums the present blocks, the colour lists hold
   nodes.
   The smoother is a coloured node-block Gauss-Seidel sweep.  A node is a scalar global dof I with its ncomp components;
   colour[i] (host, nrows nodes; read on the nodes with a free component) such that no two coupled nodes with a free component
   share a colour (checked against the pattern: IGX_ERR_ARG names the first pair).  A sweep relaxes colour after colour, one launch
   per colour; every node solves its free components exactly from its ncomp x ncomp diagonal block, the fixed ones keep their
   entry: x_F[I] = D_FF^-1 (b_F[I] - sum_{J != I} sum_q A_Fq[I,J] x_q[J] - sum_{q fixed} D_Fq x_q[I]).  A node whose elimination
   meets a zero or non-finite pivot is left as it is.  smooth_steps (1 .. 16): sweeps before and after the coarse correction. */
int  igx_solver_set_block_mg_smoother(igx_solver *solver, const int32_t *colour, int smooth_steps);
/* `coarse` becomes the next level of `solver`: two block solvers with the same number of components and patches and injective
   maps.  P and mult as in igx_solver_set_mg_coarse (those of the scalar space): every component is transferred with them on its
   slice of the vectors, under its own mask. */
int  igx_solver_set_block_mg_coarse(igx_solver *solver, igx_solver *coarse, const double *const *P, const double *mult);
/* The coarsest level: inv (host, m x m row-major, m = free dofs of `solver` in the blocked numbering, ascending). */
int  igx_solver_set_block_mg_inverse(igx_solver *solver, const double *inv, int64_t m);

/* --- Parabolic problems: DIRK time stepping on the device (pyiga/solvers.py:366-473: dirk_step with constant steps) ----------
   M u' = f - K u on the free dofs, u = g on the fixed ones, u(t0) = x0; f and g constant in time.  M is the patch's mass matrix,
   K the matrix of kind_K (any kind igx_solver_create_general accepts).  One step of the tableau A ((stages + 1) x stages, row-major,
   b the last row) from x (g on the fixed dofs):
       stage i with a_ii = 0 (i = 0 only): y_0 = x, F_0 = F of the previous step's last stage (first step: f - K x0);
       else  b_i = M x + tau sum_{j<i} a_ij F_j + tau gamma f,  R C R^T y_i = R (b_i - C ext(g)),  F_i = f - K y_i;
       x_new = y_{s-1}  (stiffly accurate).
   C = M + tau gamma K is formed once per (tau, tableau).  Every stage is one solve of the lifted system (the initial guess
   y_{i-1}) by the solver's method and preconditioner, to ||r|| <= tol ||R (b_i - C ext(g))||.  M, K and C are the solver's
   own value buffers; x, M x, y and the F_j stay on the device; a state comes down only when it is saved.  The other igx_solver_*
   calls act on C (igx_solver_spmv_d: R C R^T x; Jacobi: the diagonal of C; IGX_PRECOND_KRON: any factors, e.g. those of
   eigh(K_k, M_k) with lam'_k = tau gamma lam_k + 1/dim, the fast-diagonalization inverse of the parametric M + tau gamma K). */
enum { IGX_DIRK_MAX_STAGES = 6 };
enum { IGX_ROLE_MASS = 0, IGX_ROLE_OPERATOR = 1 };
typedef struct {
    int64_t steps;                 /* steps done */
    int32_t converged;             /* 1 if every stage solve converged (then steps = nsteps) */
    int32_t nsaved;                /* states written to `saved` */
    int64_t iterations;            /* iterations of all stage solves */
    int32_t max_stage_iterations;  /* the most iterations of one stage solve */
    int32_t reserved;
    float axpby_ms;                /* device time of forming C (the last igx_solver_set_dirk) */
    float spmv_ms;                 /* timed != 0: the M x and F = f - K y products, summed over the run */
    float combine_ms;              /* timed != 0: the stage combinations (b_i, the initial guess, y_i = x + ext(g)) */
    float solve_ms;                /* timed != 0: the stage solves */
    float total_ms;                /* device time of the whole run, transfers included */
    float reserved2;
} igx_dirk_info;
/* A parabolic solver of one whole patch (as igx_solver_create: a row slab or a span box is IGX_ERR_UNSUPPORTED; an unknown kind
   IGX_ERR_ARG).  No values are needed yet.  It starts in IGX_METHOD_CG if `symmetric` (M + tau gamma K symmetric positive
   definite), else in IGX_METHOD_BICGSTAB; IGX_METHOD_CG on a solver made with symmetric = 0 is IGX_ERR_UNSUPPORTED. */
int  igx_solver_create_parabolic(igx_patch *patch, int kind_K, int symmetric, const int64_t *fixed, int64_t nfixed, igx_solver **out);
/* Moves the values the patch holds now into the solver: IGX_ROLE_MASS takes IGX_MASS values, IGX_ROLE_OPERATOR those of kind_K
   (igx_assemble(patch, kind, algo, NULL) before each).  A hand-over of the device buffer, not a copy: the patch then holds no
   values.  A role taken twice, a patch without the values of that kind, or a buffer whose length differs from the other role's:
   IGX_ERR_ARG. */
int  igx_solver_take_values(igx_solver *solver, int role);
/* Validates the tableau A ((stages + 1) x stages, row-major, stages <= IGX_DIRK_MAX_STAGES) and the step tau, then forms
   C = M + tau gamma K on the device (k_vals_axpby).  Refused (IGX_ERR_ARG): A not lower triangular, nonzero diagonal entries that
   differ or are not positive, a zero diagonal past row 0, not stiffly accurate (b != the last stage row), tau <= 0, M or K not
   taken.  Resets the preconditioner to IGX_PRECOND_NONE (Jacobi and Kronecker depend on C): select it again. */
int  igx_solver_set_dirk(igx_solver *solver, int stages, const double *A, double tau);
/* Integrates nsteps steps of the tableau set last from x0 (host, nrows_total; its fixed entries are replaced by g).  f: host load
   vector (nrows_total); g: host values of the fixed dofs (in the order of `fixed`).  After every step k with k % save_every == 0,
   and after the last, the state (g included) goes to the next row of saved (host, rows of nrows_total).  A stage solve that does
   not converge within maxiter iterations (or breaks down) ends the run: info->converged = 0, info->steps the steps completed, and
   the state after the last completed step is saved if it was not.  stage_iters (host, nsteps x stages, or NULL) receives the
   iterations of each implicit stage.  timed != 0: events between the phases (info->spmv_ms etc.).  Deterministic: the same
   inputs give bit-identical states. */
int  igx_solver_dirk_run(igx_solver *solver, const double *f, const double *g, const double *x0, int64_t nsteps, int64_t save_every,
                         double tol, int maxiter, int check_every, int timed, double *saved, int32_t *stage_iters,
                         igx_dirk_info *info);

/* --- Adaptive steps and Rosenbrock methods: a session of attempts (pyiga/solvers.py:430-435, 475-534, 684-939) ---------------
   The number of steps is not known in advance, so the host drives the controller and the device runs one attempt per call:
       igx_solver_set_stepper, igx_solver_set_step_precond, igx_solver_step_begin, then per attempt igx_solver_step_attempt and,
       if the host accepts it, igx_solver_step_accept (and igx_solver_step_state to bring a state down).
   One attempt with the step tau from the state x (g on the fixed dofs), which it leaves untouched:
     IGX_STEPPER_DIRK        the stages of igx_solver_dirk_run; candidate x_new = y_{s-1}.  With an estimate: x_est is
                             M_ff^-1 (M_ff x + tau sum_i b^_i F_i), and M_ff x_new = M_ff x + tau sum_i b_i F_i (the last stage), so
                             R M R^T (x_est - x_new) = tau sum_i (b^_i - b_i) F_i: one CG solve on M whatever K is.
     IGX_STEPPER_ROSENBROCK  R C R^T k_i = R (f - K (x + tau sum_{j<i} (a_ij + gamma_ij) k_j)), k_i = 0 on the fixed dofs (F is affine,
                             J = -K); candidate x_new = x + tau sum b_i k_i, x_est = x + tau sum b^_i k_i.
   C = M + tau gamma K is formed again only when tau gamma differs from that of the C on the device.  The estimate is
       r = || (x_est - x_new) / (err_tol + err_tol |x|) ||_2 / sqrt(n_free)   over the free dofs (k_err_norm).
   The session owns C and the preconditioner data while it runs: after it, igx_solver_set_dirk and igx_solver_set_precond again
   before igx_solver_dirk_run or igx_solver_solve. */
enum { IGX_STEPPER_DIRK = 0, IGX_STEPPER_ROSENBROCK = 1 };
enum { IGX_STEP_STATE = 0, IGX_STEP_CANDIDATE = 1 };
typedef struct {
    double  r;                     /* the error ratio (0 without an estimate or when a solve did not converge) */
    int32_t converged;             /* 1 if every solve of the attempt converged: there is a candidate */
    int32_t reformed;              /* 1 if C was formed again for this tau */
    int32_t has_estimate;          /* 1 if err_tol > 0 */
    int32_t mass_iterations;       /* iterations of the mass solve of an embedded DIRK rule */
    int32_t stage_iterations[IGX_DIRK_MAX_STAGES];   /* per stage (0: explicit, or not reached) */
    int64_t n_free;
    float axpby_ms;                /* forming C, if it was formed */
    float spmv_ms;                 /* timed != 0: the products with M and K */
    float combine_ms;              /* timed != 0: right-hand sides, initial guesses, the candidate */
    float solve_ms;                /* timed != 0: the stage solves */
    float mass_ms;                 /* timed != 0: the mass solve */
    float err_ms;                  /* timed != 0: k_err_norm, its finish and the read-back */
    float total_ms;                /* device time of the whole attempt */
    float reserved;
} igx_step_info;
/* The scheme of the session.  IGX_STEPPER_DIRK: A as igx_solver_set_dirk takes it ((stages + 1) x stages, the same conditions),
   Gamma NULL, b NULL or equal to the last row of A.  IGX_STEPPER_ROSENBROCK: A and Gamma stages x stages, A strictly lower
   triangular, Gamma lower triangular with one positive diagonal value gamma, b of stages weights.  b_hat: the weights of the
   embedded rule, or NULL (no estimate).  Anything else: IGX_ERR_ARG.  Ends a running session. */
int  igx_solver_set_stepper(igx_solver *solver, int family, int stages, const double *A, const double *Gamma, const double *b,
                            const double *b_hat);
/* The preconditioner of the session's solves: IGX_PRECOND_NONE, IGX_PRECOND_JACOBI (the diagonal of the values in use, by k_diag)
   or IGX_PRECOND_KRON with the factors U_k and the RAW eigenvalues lam_k of eigh(K_k, M_k) on the free box (arguments as
   igx_solver_set_precond's).  The device rewrites the eigenvalue slots per attempt: tau gamma lam_k + 1/dim for C, 1/dim for M
   (U_k^T M_k U_k = I: the inverse of the parametric mass matrix).  A change of step uploads nothing.  igx_solver_set_precond
   replaces the factors: call this again after it. */
int  igx_solver_set_step_precond(igx_solver *solver, int precond, const int32_t *box_lo, const int32_t *box_hi,
                                 const double *const *U, const double *const *lam_raw);
/* Starts a session: f, g and x0 as igx_solver_dirk_run takes them, the only uploads of vectors. */
int  igx_solver_step_begin(igx_solver *solver, const double *f, const double *g, const double *x0);
/* One attempt.  err_tol <= 0: no estimate (constant steps; required if the scheme has no b_hat).  Every solve runs to
   ||r|| <= solve_tol ||r0|| within maxiter iterations, r0 the residual of its start value: zero (r0 the right-hand side) but for
   the DIRK stages, which start from y_{i-1} and so are solved for their increment (the reference's Newton measures rtol the same
   way); a start value that meets solve_tol ||rhs|| already is taken as it is.  A solve that does not converge ends the attempt
   with info->converged = 0 (no candidate; the host rejects and halves tau).  The state and, for an explicit first stage, F_1 are
   untouched by the attempt. */
int  igx_solver_step_attempt(igx_solver *solver, double tau, double err_tol, double solve_tol, int maxiter, int check_every,
                             int timed, igx_step_info *info);
/* The candidate of the last attempt becomes the state (a swap of pointers). */
int  igx_solver_step_accept(igx_solver *solver);
/* The state (IGX_STEP_STATE) or the candidate of the last attempt (IGX_STEP_CANDIDATE), g included, to the host. */
int  igx_solver_step_state(igx_solver *solver, int which, double *out);
/* k_err_norm alone on device vectors of the solver's length (any solver):
   *r = || (sum_k coef[k] d_v[k]) / (tol + tol |d_x|) ||_2 / sqrt(n_free) over the free dofs; nv from 1 to 8. */
int  igx_solver_error_ratio_d(igx_solver *solver, int nv, const double *coef, const double *const *d_v, const double *d_x,
                              double tol, double *r);

/* --- Generalized eigenproblems: the pieces of a block LOBPCG for K x = lam M x ------------------------
   On a solver made by igx_solver_create_parabolic (symmetric) that has taken M and K (igx_solver_take_values); no C is needed.
   A block holds m <= 16 vectors of all dofs, row-major with the columns interleaved: entry (I, j) at I * mb + j, mb the row
   stride: 4, 8 or 16, the smallest of them >= m.  Padding columns are zero and never enter a Gram matrix; the rows of fixed dofs
   are zero.  The host drives the iteration (Gram matrices and norms come down, coefficient matrices go up); the device keeps the
   blocks of a session under the ids below.  Every reduction has a fixed order and no atomics: the same calls give the same bits.
       igx_solver_eig_set_precond, igx_solver_eig_begin, then products / gram / combine / residuals / precond in any order,
       igx_solver_eig_download, igx_solver_eig_info, igx_solver_eig_end.
   Calls on a solver that is not such a parabolic one, or (but for set_precond and the _d calls) outside a session: IGX_ERR_ARG.
   A multipatch solver (igx_solver_create_multipatch) that has been given a mass matrix (igx_solver_set_mass_d) is accepted as
   well: K is the multipatch's summed values (restarted sums: IGX_ERR_ARG, as for every call on such a
   solver), M the solver's own array, the block product k_csr_spmm2 over the global CSR pattern, nrows_total the global dofs.
   Without a mass matrix: IGX_ERR_ARG.
   A block solver (igx_solver_create_block with symmetric != 0) whose diagonal blocks are all present and that has taken a mass
   matrix (igx_solver_take_mass) is accepted too: the vector-valued eigenproblem K x = lam (I (x) M) x, K
   the ncomp x ncomp blocks, M one scalar matrix for every component.  Blocks then have ncomp * nrows_total rows, component-major
   (entry (q N + J, j) at (q N + J) mb + j); the block product is k_block_spmm2, every other entry works on the longer blocks
   unchanged.  A block solver that is not symmetric: the message of every other solver; a missing diagonal block or mass:
   IGX_ERR_ARG. */
enum { IGX_EIG_X = 0, IGX_EIG_KX, IGX_EIG_MX, IGX_EIG_W, IGX_EIG_KW, IGX_EIG_MW, IGX_EIG_P, IGX_EIG_KP, IGX_EIG_MP, IGX_EIG_R,
       IGX_EIG_NBLOCKS };
typedef struct {
    int32_t m, mb;                 /* columns and row stride of the session's blocks */
    int32_t products;              /* block products (k_spmm2 launches) */
    int32_t grams, combines, residuals, preconds;    /* launches of the other phases */
    int32_t reserved;
    int64_t n_free;
    float products_ms;             /* timed != 0: device time per phase, summed over the session */
    float gram_ms;
    float combine_ms;
    float residual_ms;
    float precond_ms;
    float reserved2;
} igx_eig_info;
/* The second matrix of a multipatch solver: d_M holds nnz values in the order of igx_multipatch_pattern, allocated with
   igx_dev_alloc on the solver's context.  The solver takes ownership: it frees d_M when it is destroyed, and a second call frees
   the array of the first.  A patch solver: IGX_ERR_UNSUPPORTED. */
int  igx_solver_set_mass_d(igx_solver *solver, double *d_M);
/* The mass matrix of a block solver's eigenproblem: the patch's current values (IGX_MASS, or IGX_FORM for a density-weighted
   mass) change hands as a block does (igx_solver_take_block); the solver frees them in igx_solver_destroy.  A second call, a
   solver that is not a block solver, or a patch without such values: IGX_ERR_ARG. */
int  igx_solver_take_mass(igx_solver *solver);
/* The preconditioner of igx_solver_eig_precond and igx_solver_eig_precond_d: IGX_PRECOND_NONE (the masked copy),
   IGX_PRECOND_JACOBI (the diagonal of K) or IGX_PRECOND_KRON with factors as igx_solver_set_precond takes them (the free dofs must
   be exactly the box).  Independent of igx_solver_set_precond.  A multipatch solver takes NONE, JACOBI or IGX_PRECOND_MG: one
   V-cycle of the hierarchy of igx_solver_set_mg_* per column (not set up: IGX_ERR_ARG; the _d form cycles all mb columns, a
   session the first m); IGX_PRECOND_KRON and IGX_PRECOND_SCHWARZ: IGX_ERR_UNSUPPORTED.  A block solver: JACOBI is the diagonal
   of every diagonal block; KRON takes NULL box arguments and applies the factors of igx_solver_set_block_kron per component, on
   that component's box with all mb columns at once (a component without factors, or box arguments: IGX_ERR_ARG; factors set
   again later: select KRON again). */
int  igx_solver_eig_set_precond(igx_solver *solver, int precond, const int32_t *box_lo, const int32_t *box_hi,
                                const double *const *U, const double *const *lam, int lam_mode);
/* Starts a session with blocks of m columns (1 <= m <= 16): X0 (host, nrows_total x m, row-major) goes into IGX_EIG_X with its
   fixed rows cleared, every other block is cleared.  timed != 0: events around every phase (igx_eig_info). */
int  igx_solver_eig_begin(igx_solver *solver, int m, const double *X0, int timed);
/* dst_K = R K R^T src and dst_M = R M R^T src in one pass over both value arrays (k_spmm2); dst_K or dst_M < 0: the other
   matrix alone.  src must differ from both. */
int  igx_solver_eig_products(igx_solver *solver, int src, int dst_K, int dst_M);
/* G = [A_0 .. A_{na-1}]^T [B_0 .. B_{nb-1}] over the free dofs (na, nb from 1 to 3; k_gram and its finish) to the host:
   (na m) x (nb m), row-major. */
int  igx_solver_eig_gram(igx_solver *solver, int na, const int32_t *a, int nb, const int32_t *b, double *G);
/* nupd (1 or 2) combinations: block dst[u] = sum_{j < nsrc[u]} block src[3 u + j] . coef[(3 u + j) m m ..] (m x m, row-major:
   entry (a, b) takes column a of the source into column b), nsrc[u] from 1 to 3.  triple != 0: dst and src name blocks among
   X, W, P and the same combination is applied to their K and M companions.  Every source is read before any destination is
   written (the results go to scratch blocks whose pointers are swapped in): a destination may be among the sources. */
int  igx_solver_eig_combine(igx_solver *solver, int nupd, const int32_t *dst, const int32_t *nsrc, const int32_t *src,
                            const double *coef, int triple);
/* IGX_EIG_R = KX - MX diag(lam) (lam: host, m) and, in the same kernel, the column 2-norms of R and of KX over the free dofs
   (host, m each). */
int  igx_solver_eig_residuals(igx_solver *solver, const double *lam, double *rnorm, double *knorm);
/* block dst = T block src, column by column, T the preconditioner of igx_solver_eig_set_precond; src != dst. */
int  igx_solver_eig_precond(igx_solver *solver, int src, int dst);
/* The first k <= m columns of a block to the host (nrows_total x k, row-major). */
int  igx_solver_eig_download(igx_solver *solver, int block, int k, double *out);
int  igx_solver_eig_info(igx_solver *solver, igx_eig_info *info);
/* Ends the session and frees its blocks (the preconditioner set last stays). */
int  igx_solver_eig_end(igx_solver *solver);
/* The pieces on device buffers of nrows_total * mb doubles (mb 4, 8 or 16; 16-byte aligned), outside any session.
   products_d: d_X is masked first (a copy), then d_YK = R K R^T X and d_YM = R M R^T X; one of them may be NULL.
   gram_d: as igx_solver_eig_gram with the first m columns of the blocks d_A[0..na) and d_B[0..nb).
   combine_d: d_Y = sum_{j < nsrc} d_S[j] . coef[j] (coef: host, nsrc x m x m); d_Y must not be a source.
   residuals_d: d_R = d_KX - d_MX diag(lam) and the two column norms (m each).
   precond_d: d_Z = T d_R; different buffers. */
int  igx_solver_eig_products_d(igx_solver *solver, int mb, const double *d_X, double *d_YK, double *d_YM);
int  igx_solver_eig_gram_d(igx_solver *solver, int mb, int m, int na, const double *const *d_A, int nb, const double *const *d_B,
                           double *G);
int  igx_solver_eig_combine_d(igx_solver *solver, int mb, int m, int nsrc, const double *const *d_S, const double *coef,
                              double *d_Y);
int  igx_solver_eig_residuals_d(igx_solver *solver, int mb, int m, const double *d_KX, const double *d_MX, const double *lam,
                                double *d_R, double *rnorm, double *knorm);
int  igx_solver_eig_precond_d(igx_solver *solver, int mb, const double *d_R, double *d_Z);

/* Kronecker product  y = D^-1 (B_0 (x) B_1 [(x) B_2]) x  on device buffers. The factors are dense, row-major, m[k] x n[k]
   (rectangular allowed).  x and y are tensors of shape (n_0, .., n_{dim-1}, batch) and (m_0, .., batch), addressed through an
   element offset and four strides (axis 3 = the trailing batch axis), so a sub-box of a longer vector can be read or written.
   D: lam_mode 0 none, IGX_KRON_SUM / IGX_KRON_PRODUCT of d_lam[k] (m[k] each) at the output index.  d_work: 2 * W doubles with
   W = max over k < dim - 1 of batch * m_0 .. m_k * n_{k+1} .. n_{dim-1}, or NULL (allocated for the call).  x and y must not
   overlap.  Returns when the result is in y. */
typedef struct {
    int32_t dim;                       /* 1..3 factors */
    int32_t m[3], n[3];
    const double *d_B[3];
    int64_t batch;                     /* >= 1 */
    int64_t x_off, x_stride[4];        /* x(i_0, .., t) = d_x[x_off + sum_k i_k x_stride[k] + t x_stride[3]] */
    int64_t y_off, y_stride[4];
    int32_t lam_mode;
    int32_t reserved;
    const double *d_lam[3];
} igx_kron_desc;
int igx_kron_apply_d(igx_ctx *ctx, const igx_kron_desc *desc, const double *d_x, double *d_y, double *d_work, int64_t work_len);

/* Bilinear forms over TWO spline spaces on one mesh (Taylor-Hood, Q1-P0, ..: pyiga's assemble(problem, (kvs0, kvs1), bfuns=
   [('u', nc, 0), ('p', nc, 1)])).  A pair is a full patch -- the TRIAL space (columns; space 0 of the reference), which owns the
   geometry, the Gauss grid and the form fields -- plus a TEST space (rows; space 1) given by per-axis degree and open knot
   vector.  The patch's quadrature is used as it is: create the patch with nqp = max degree over BOTH spaces + 1, the
   reference's rule.  The matrix is prod(ndofs_test) x prod(ndofs_trial), canonical CSR holding exactly the product pattern:
   row (i0, i1[, i2]) has the columns [jlo_0, jhi_0) x [jlo_1, jhi_1) [x ..] in lexicographic order, [jlo_k, jhi_k) the trial
   functions of axis k whose mesh support meets that of test function i_k.
   igx_pair_create returns NULL (igx_last_error names the condition) unless: the test space has the patch's dim; its degrees
   are <= IGX_MAX_DEGREE and its knot vectors open; per axis its breakpoints equal the patch's exactly; the patch is whole (no
   span box, no row slab, not an internal twin) and its basis tables hold (value, first derivative).  The patch must outlive
   the pair. */
typedef struct igx_pair igx_pair;
typedef struct {
    int32_t dim, reserved;
    int32_t ndofs_trial[IGX_MAX_DIM], ndofs_test[IGX_MAX_DIM];
    int64_t nrows, ncols, nnz;         /* prod(ndofs_test), prod(ndofs_trial), entries of the pattern */
} igx_pair_info;
igx_pair *igx_pair_create(igx_patch *patch, int dim, const int32_t *p, const int32_t *kv_len, const double *const *kv);
void igx_pair_destroy(igx_pair *pair);
int  igx_pair_get_info(const igx_pair *pair, igx_pair_info *info);
/* indptr: nrows + 1 entries, indices: nnz global column ids; either may be NULL; kept on the device.  IGX_ERR_UNSUPPORTED
   for nnz or ncols >= 2^31 (int32 indices) -- never a truncated pattern. */
int  igx_pair_pattern(igx_pair *pair, int32_t *indptr, int32_t *indices);
/* All nnz values in the order of igx_pair_pattern, one thread per entry in the reference's summation order; kept on the
   device (igx_pair_d_data) and copied to data_out if it is not NULL.  kind: IGX_MASS, or IGX_FORM with the physical table of
   igx_patch_set_form[_d|_expr] (a parametric jet form: IGX_ERR_UNSUPPORTED).  The fields are the patch's own: they depend on
   geometry and coefficients only.  A launch beyond the grid limit is IGX_ERR_UNSUPPORTED. */
int  igx_pair_assemble(igx_pair *pair, int kind, double *data_out);
/* ij: M x 2 (row = ravelled test dof, column = ravelled trial dof), host in and out; disjoint supports or an index at or
   past the row / column count give exactly 0.0.  The values have the bits of the corresponding igx_pair_assemble values. */
int  igx_pair_entries(igx_pair *pair, int kind, const size_t *ij, size_t M, double *out);
const double *igx_pair_d_data(const igx_pair *pair);     /* values of the last igx_pair_assemble (NULL before the first) */
/* Device times of the last igx_pair_assemble: total_ms, fields_ms (0 when the patch still held the fields), entry_ms. */
int  igx_pair_last_timing(const igx_pair *pair, igx_timing *t);

/* --- Saddle-point systems  [[A, B^T], [B, 0]]  (Stokes) solved on the device with preconditioned MINRES ---
   A: the nc x nc blocks of a vector-valued form over `patch_u` (velocity, N_u dofs per component), B = [B_0 .. B_{nc-1}]: the
   values of `pair` (rows: its test space, the pressure, N_p dofs; columns: patch_u).  Vectors have nc * N_u + N_p entries, the
   velocity components first, component-major.  The solver is a block solver with a pressure part: A is taken block by block with
   igx_solver_take_block, B with igx_solver_take_pair_block; igx_solver_solve, igx_solver_spmv_d (R K R^T x), igx_solver_precond_d,
   igx_solver_set_block_kron, igx_solver_set_precond and igx_solver_last_breakdown serve it.  Its method is IGX_METHOD_MINRES
   (Paige and Saunders; any other: IGX_ERR_UNSUPPORTED): it stops at phi_k <= tol * phi_0, phi MINRES's own estimate of
   sqrt(r^T P r), read back every check_every iterations; info->relres is the true ||R (b - K u)|| / ||R (b - K ext(g))|| from one
   more product.  A non-finite scalar (IGX_BREAKDOWN_NONFINITE) or r.(P r) < 0 (IGX_BREAKDOWN_INDEFINITE_PRECOND) stops the solve
   without converging; u is then the last finite iterate.  Two solves of one system are bit-identical, whatever check_every.
   The eigen, parabolic, stepping, Newton and multigrid calls: IGX_ERR_UNSUPPORTED.

   ncomp = 2 or 3 and a pair made over patch_u (else IGX_ERR_ARG); fixed[0..nfixed) index all nc * N_u + N_p entries. */
int  igx_solver_create_saddle(igx_patch *patch_u, igx_pair *pair, int ncomp, const int64_t *fixed, int64_t nfixed, igx_solver **out);
/* The values the pair holds now (igx_pair_assemble, IGX_FORM or IGX_MASS) become B_q: the device buffer changes hands
   (igx_pair_d_data is NULL afterwards, the next assembly allocates anew), and B_q^T is formed on the device in the pair layout
   of the swapped spaces (k_pair_transpose: an exact copy of the bits).  A block taken twice, q out of range, a pair other than
   the solver's or one without values: IGX_ERR_ARG.  A product or a solve needs every B_q and the diagonal blocks of A. */
int  igx_solver_take_pair_block(igx_solver *solver, igx_pair *pair, int q);
/* The pressure part of the block-diagonal preconditioner diag(P_0, .., P_{nc-1}, P_S), selected with the rest by
   igx_solver_set_precond(IGX_PRECOND_KRON | _JACOBI | _NONE; box and factor arguments NULL).  mode IGX_PRECOND_KRON: scale times
   the fast-diagonalization inverse (lam_mode IGX_KRON_PRODUCT: (x) M_k^-1) on the box box_lo[k] <= i_k < box_hi[k] of the
   pressure space (factors as igx_solver_set_precond's), applied to the masked vector and masked again, so that it stays positive
   definite with a pinned dof.  mode IGX_PRECOND_JACOBI: scale times dinv (host, N_p entries; the box and factor arguments are not
   read; its entries are not checked: a negative one makes the preconditioner indefinite, which the solve reports as
   IGX_BREAKDOWN_INDEFINITE_PRECOND).  The velocity part: igx_solver_set_block_kron per component (KRON) or the diagonals of the
   A_cc (JACOBI).  scale (positive, else IGX_ERR_ARG): the viscosity nu of  -nu Laplace u.  The call resets the preconditioner to
   IGX_PRECOND_NONE, also when it fails: select it again with igx_solver_set_precond. */
int  igx_solver_set_saddle_schur(igx_solver *solver, int mode, const int32_t *box_lo, const int32_t *box_hi, const double *const *U,
                                 const double *const *lam, int lam_mode, const double *dinv, double scale);
/* enable >= 0: whether the following solves remove the mean of the pressure part of the lifted right-hand side (the orthogonal
   projection onto the range of a system whose kernel is the constant pressure: every velocity dof of the boundary fixed, no
   pressure dof fixed; with a fixed pressure dof IGX_ERR_ARG) -- the final residual is projected alike; enable < 0: unchanged.
   mean / norm (either may be NULL): that mean and the norm of that pressure part at the last solve. */
int  igx_solver_saddle_projection(igx_solver *solver, int enable, double *mean, double *norm);
/* Inspection calls of a saddle-point solver: no workflow needs them; the tests of the kernels and tools/saddle_timing.py do.
   igx_solver_download_pair_block: the nnz values of B_q (transposed = 0: in the order of igx_pair_pattern) or of B_q^T
   (transposed != 0: in the pair layout of the swapped spaces, i.e. in the order of the canonical CSR of the transposed matrix) to
   the host.  An absent block: IGX_ERR_ARG.
   igx_solver_saddle_product_d: one product with the whole contract of the row kernels, as the lifting and the MINRES iterations
   call them: d_y = free ? (d_b ? d_b : 0) + sign * K d_x : 0 over all nc N_u + N_p rows (d_x is NOT masked; d_b may be NULL;
   d_x and d_y different buffers), and with d_pd not NULL the kernels' dot partials of d_pd . d_y, added up in their fixed order
   into *dot (dot may be NULL).  The two launches are timed apart.
   igx_solver_saddle_timing: device ms of the last k_pair_transpose (igx_solver_take_pair_block) and of the velocity-row and the
   pressure-row launch of the last igx_solver_saddle_product_d; any pointer may be NULL. */
int  igx_solver_download_pair_block(const igx_solver *solver, int q, int transposed, double *vals);
int  igx_solver_saddle_product_d(igx_solver *solver, const double *d_x, const double *d_b, double sign, const double *d_pd, double *d_y,
                                 double *dot);
int  igx_solver_saddle_timing(const igx_solver *solver, float *transpose_ms, float *u_rows_ms, float *p_rows_ms);

/* --- Restarted GMRES on a saddle-point solver: Oseen systems  [[nu A + N(w), B^T], [B, 0]]   ---
   The velocity blocks taken with igx_solver_take_block may form a non-symmetric matrix (a frozen-wind convection term added to
   the viscous one); MINRES is then the wrong method, and this call selects right-preconditioned GMRES(restart) for the
   following igx_solver_solve calls.  The solver's method stays IGX_METHOD_MINRES: that constant names the solver family
   (saddle-point), which igx_solver_set_method guards; the Krylov method within the family is chosen here.
   restart in 1..128 (else IGX_ERR_ARG): the basis of (restart + 1) * n doubles and the small arrays (Hessenberg column,
   rotations, g, y, the triangular factor) are allocated once, and again only for a larger restart.  restart = 0 returns to MINRES
   and frees nothing.  triangular != 0: igx_solver_set_precond's KRON or JACOBI parts are applied as the block upper-triangular
   preconditioner, the solve with [[F, B^T], [0, -S]] -- z_p = -P_S r_p, z_u = P_F (r_u - B^T z_p) -- instead of diag(P_F, P_S),
   also by igx_solver_precond_d; it is not symmetric, so with restart = 0 it is IGX_ERR_ARG.  Any solver that is not a
   saddle-point solver: IGX_ERR_UNSUPPORTED.
   The solve stops at |g_{j+1}| <= tol * ||r0||, GMRES's own residual norm, read back every check_every steps and at the end of
   every cycle; at a restart the residual is formed again with a product.  info->iterations counts Arnoldi steps, info->relres is
   the true relative residual as for MINRES.  h_{j+1,j} = 0 (the lucky breakdown) counts as converged; a non-finite scalar stops
   the solve with IGX_BREAKDOWN_NONFINITE before any update of u by that cycle.  Two solves are bit-identical, whatever
   check_every. */
int  igx_solver_set_gmres(igx_solver *solver, int restart, int triangular);
/* Restarts of the last GMRES solve (cycles after the first). */
int  igx_solver_gmres_restarts(const igx_solver *solver);
/* Inspection calls of GMRES: no workflow needs them; the tests of the kernels and tools/oseen_timing.py do.  All need GMRES
   selected, and 1 <= ncols <= restart + 1.
   igx_solver_gmres_orth_d: one full orthogonalisation (classical Gram-Schmidt twice) of d_w (n entries, overwritten) against the
   first ncols columns of d_V (leading dimension n), the kernels of an Arnoldi step in their order; h_out (host, ncols doubles):
   the coefficients h_k, the sums of both passes; norm_out: ||w|| afterwards.  Either may be NULL.
   igx_solver_gmres_combine_d: d_t = sum_{k < ncols} y[k] d_V[:, k] (y on the host), the kernel of the update of x.
   igx_solver_gmres_timing: the mean device ms of an orthogonalisation (with the scalars and the scale of the step) and of an
   update of x (back substitution, combination, preconditioner, add) over the last timed solve -- or of the last of the two calls
   above; any pointer may be NULL. */
int  igx_solver_gmres_orth_d(igx_solver *solver, const double *d_V, int ncols, double *d_w, double *h_out, double *norm_out);
int  igx_solver_gmres_combine_d(igx_solver *solver, const double *d_V, int ncols, const double *y, double *d_t);
int  igx_solver_gmres_timing(const igx_solver *solver, float *orth_ms, float *combine_ms);

/* --- The correction form of a nonlinear iteration on a saddle-point solver running GMRES (stationary Navier-Stokes: Picard and
   Newton steps).  igx_solver_newton_update_d's siblings: that call serves scalar patch solvers only.
   The iterate d_x (nc N_u + N_p doubles, Dirichlet values included) is the caller's device vector from the first step to the last.
   igx_solver_saddle_residual_d: r = R (d_b - K d_x) by the row kernels (igx_solver_saddle_product_d's contract; d_b may be NULL),
   its pressure mean removed if the solver projects (igx_solver_saddle_projection); r stays in the solver, *norm receives ||r||,
   the one scalar that comes down.
   igx_solver_saddle_correct_d: d_x += K^-1 r with the blocks the solver holds NOW -- they may have been replaced since the
   residual was formed (igx_solver_replace_block: Newton forms the residual with the Picard blocks and solves with the Newton
   blocks) -- by GMRES from zero with zero Dirichlet values to |g_k| <= tol * ||r||; info as igx_solver_solve's.
   A solver that is not a saddle-point solver: IGX_ERR_ARG; MINRES selected: IGX_ERR_UNSUPPORTED. */
int  igx_solver_saddle_residual_d(igx_solver *solver, const double *d_b, const double *d_x, double *norm);
int  igx_solver_saddle_correct_d(igx_solver *solver, double *d_x, double tol, int maxiter, int check_every, int timed,
                                 igx_solve_info *info);

/* --- Hierarchical (HB / THB) spline spaces: the level-coupling contraction (pyiga_amd/hierarchical.py).
   The entry of the HB matrix between the active function a of level la and the active function b of level k >= la is
       A[a, b] = sum_i W[i, a] A_k[i, b],      A[b, a] = sum_i A_k[b, i] W[i, a],
   A_k the tensor-product matrix of level k, W = (x)_axes of the composite two-scale matrices from level la to level k, i over
   the children of a on level k whose support overlaps that of b.  One block = the work items of one pair of levels.
   Per axis: d_clo / d_ccnt / d_w[n_coarse][wmax] -- first child, number of children and weights of every coarse function
   (la == k: clo[a] = a, one child, weight 1); d_first / d_cnt -- per function of level k the first overlapping function of level
   k and their number; box_lo / box_n -- the range of dof indices the row-slot map covers.
   d_slot[prod box_n]: the slot of a row of level k, -1 without; the entries of row slot s start at d_rowptr[s] and hold its
   tensor-product stencil, columns d_first .. + d_cnt per axis, last axis fastest: the order igx_entries_d fills them in.
   Work item n: d_ia[n], d_ib[n] the ravelled indices of a and b on their levels, d_pos[n] the position of A[a, b] and
   d_pos2[n] (-1: none) the position of A[b, a] in d_values.  symmetric != 0: A[b, a] is a copy of A[a, b]; else it is summed
   in the other orientation.  `group` lanes (16 or 64) sum the terms of one item in a fixed order: no atomics, the values are
   the same bits in every run and for every grid.  max_blocks > 0 caps the grid (0: the library's default).  A term that would
   read outside the slot map or the entries yields NaN; a position outside [0, nnz) is not written. */
typedef struct {
    const int32_t *d_clo, *d_ccnt;
    const double  *d_w;
    const int32_t *d_first, *d_cnt;
    int32_t wmax, n_coarse, n_fine, box_lo, box_n, reserved;
} igx_hier_axis;
typedef struct {
    int32_t dim, symmetric;
    igx_hier_axis ax[IGX_MAX_DIM];
    const int32_t *d_slot;
    const int64_t *d_rowptr;
    const double  *d_entries;
    int64_t n_entries;
    const int32_t *d_ia, *d_ib, *d_pos, *d_pos2;
    int64_t n_items;
    int32_t group, max_blocks;
} igx_hier_block;
/* *ms (may be NULL): the device time of the kernel from events; the call then waits for it. */
int  igx_hier_contract_d(igx_ctx *ctx, const igx_hier_block *block, double *d_values, int64_t nnz, float *ms);
/* d_dst[n] = d_src[d_idx[n]], n < n_idx: the active entries of a level's vector in canonical order (an index outside
   [0, n_src) yields NaN). */
int  igx_hier_gather_d(igx_ctx *ctx, const double *d_src, int64_t n_src, const int64_t *d_idx, int64_t n_idx, double *d_dst);

/* --- Local multigrid for hierarchical spline spaces (pyiga/solvers.py:174-324: local_mg_step,
   iterative_solve, solve_hmultigrid).  All CSR matrices have int32 pointers and columns.
   igx_csr_rap_d: the values of C = P^T A P on the given pattern of C (n_c x n_c), everything on the device.  A is n_f x n_f and
   need not be symmetric; the columns of each of its rows ascend (an entry the bisection does not find is no term).  P is given
   by its transpose alone, P^T (n_c x n_f, rows in any order): column j of P is row j of P^T.  pt_row_max: the longest row of
   P^T (it selects the lane group: 4, 16 or 64 lanes own one output entry).  Term t = a |row j| + b of C[i, j] is
   (P^T[i, k_a] A[k_a, m_b]) P^T[j, m_b], a and b the positions in the rows i and j of P^T; lane l of the group adds the terms
   l, l + G, .. in ascending order and a shuffle tree of fixed shape adds the lanes: no atomics, the same bits in every run and for
   every grid.  max_blocks > 0 caps the grid (0: the library's default).  A position of the pattern without terms is written as
   exactly 0.0; an index outside its array makes the entry NaN instead of a read.  Not waited for. */
int  igx_csr_rap_d(igx_ctx *ctx, int64_t n_f, int64_t n_c, const int32_t *d_a_indptr, const int32_t *d_a_indices, const double *d_a_vals,
                   int64_t a_nnz, const int32_t *d_pt_indptr, const int32_t *d_pt_indices, const double *d_pt_vals, int64_t pt_nnz,
                   int32_t pt_row_max, const int32_t *d_c_indptr, const int32_t *d_c_indices, double *d_c_vals, int64_t c_nnz,
                   int32_t max_blocks);
/* d_y = M d_x (accumulate == 0) or d_y += M d_x for a rectangular CSR matrix (nrows x ncols) on the device: a group of lanes per
   row (its width from row_max, the longest row, as the CSR SpMV of the solvers chooses it), fixed summation order.  A column
   outside [0, ncols) or a row range outside [0, nnz] makes the row NaN instead of a read.  Not waited for. */
int  igx_csr_rect_spmv_d(igx_ctx *ctx, int64_t nrows, int64_t ncols, const int32_t *d_indptr, const int32_t *d_indices, const double *d_vals,
                         int64_t nnz, int32_t row_max, const double *d_x, double *d_y, int accumulate, int32_t max_blocks);

/* The handle that owns a hierarchy: level 0 the coarsest, nlevels - 1 the finest.  Set-up order: igx_hmg_set_matrix for every
   level (the finest with its values), igx_hmg_set_transfer for the levels > 0, igx_hmg_galerkin from the finest level down,
   igx_hmg_set_smoother for the levels > 0, igx_hmg_set_inverse, igx_hmg_set_free. */
typedef struct igx_hmg igx_hmg;
#define IGX_HMG_MAX_LEVELS 16
enum { IGX_HMG_GS = 0,            /* forward sweeps before the coarse correction, backward sweeps after it */
       IGX_HMG_FORWARD_GS = 1, IGX_HMG_BACKWARD_GS = 2,
       IGX_HMG_SYMMETRIC_GS = 3 };/* a forward and a backward sweep per step, before and after */
enum { IGX_HMG_ITERATE = 0,       /* x <- cycle(x) until the residual over the free dofs has dropped by tol */
       IGX_HMG_CG = 1 };          /* CG on the free dofs with one cycle from a zero guess as preconditioner (gs, symmetric_gs) */
typedef struct {
    int32_t iterations;           /* cycles (iterate) or CG steps done */
    int32_t converged;            /* 1 if ratio < tol was reached */
    double ratio;                 /* final ||(f - A x)[free]|| / ||f[free]|| (CG: of the recurrence residual) */
    int64_t n_free;
} igx_hmg_info;
typedef struct {
    int32_t levels, launches;     /* kernel launches of one cycle */
    float total_ms, coarse_ms;    /* device time of one cycle (mean over reps) and of the dense solve of level 0 */
    float smooth_ms[IGX_HMG_MAX_LEVELS], residual_ms[IGX_HMG_MAX_LEVELS], transfer_ms[IGX_HMG_MAX_LEVELS];   /* per level */
} igx_hmg_profile;
typedef struct {
    int64_t nrows, nnz, nsmooth;  /* nsmooth: rows of the smoothing set (level 0: of the dense inverse) */
    int32_t ncolours, one_block, group_width, reserved;
} igx_hmg_level;
int  igx_hmg_create(igx_ctx *ctx, int nlevels, igx_hmg **out);
void igx_hmg_destroy(igx_hmg *h);
/* The pattern of level `level` (host arrays; columns ascending within a row) and its values: d_vals (device, nnz doubles, copied)
   or NULL for a level whose values igx_hmg_galerkin computes. */
int  igx_hmg_set_matrix(igx_hmg *h, int level, int64_t n, const int32_t *indptr, const int32_t *indices, const double *d_vals);
/* The prolongation P of level `level` > 0 from level - 1 (host CSR, n_level x n_c); P^T is formed on the host. */
int  igx_hmg_set_transfer(igx_hmg *h, int level, int64_t n_c, const int32_t *indptr, const int32_t *indices, const double *vals);
/* A_{level-1} = P^T A_level P by igx_csr_rap_d's kernel on the pattern level - 1 was given. */
int  igx_hmg_galerkin(igx_hmg *h, int level, int32_t max_blocks);
/* The smoothing set of level `level` > 0: rows sorted by (colour, index), colour c = rows[colour_offsets[c] ..
   colour_offsets[c + 1]).  Two coupled rows of one colour are IGX_ERR_ARG.  A set of at most block_rows rows sweeps in one
   launch of one block, a larger one with one launch per colour. */
int  igx_hmg_set_smoother(igx_hmg *h, int level, int32_t ncolours, const int32_t *colour_offsets, const int32_t *rows, int64_t block_rows);
/* Level 0: x[ind[i]] = sum_j inv[i][j] f[ind[j]], inv the m x m row-major inverse of A_0[ind, ind] (host arrays). */
int  igx_hmg_set_inverse(igx_hmg *h, const int32_t *ind, int64_t m, const double *inv);
int  igx_hmg_set_options(igx_hmg *h, int smoother, int smooth_steps);
/* free_mask[i] != 0: dof i of the finest level counts in the residual norm (the non-Dirichlet dofs). */
int  igx_hmg_set_free(igx_hmg *h, const uint8_t *free_mask);
int  igx_hmg_level_values(igx_hmg *h, int level, double *out);        /* the values of a level's matrix, to the host */
int  igx_hmg_level_info(igx_hmg *h, int level, igx_hmg_level *out);
/* d_y = [d_b +] sign A d_x with the matrix of the finest level (d_b may be NULL, or d_y); not waited for. */
int  igx_hmg_spmv_d(igx_hmg *h, const double *d_x, const double *d_b, double sign, double *d_y);
/* d_x <- one cycle with the right-hand side d_f (the reference's step(x)); one stream, no host round trip; not waited for. */
int  igx_hmg_cycle_d(igx_hmg *h, const double *d_f, double *d_x);
/* Solves A x = f from x = 0 (device vectors of the finest level).  IGX_HMG_CG with a smoother other than gs / symmetric_gs:
   IGX_ERR_UNSUPPORTED. */
int  igx_hmg_solve_d(igx_hmg *h, int method, const double *d_f, double *d_x, double tol, int maxiter, igx_hmg_info *info);
/* `reps` cycles on d_x with events after every phase. */
int  igx_hmg_profile_d(igx_hmg *h, const double *d_f, double *d_x, int reps, igx_hmg_profile *out);

#ifdef __cplusplus
}
#endif
#endif /* IGX_H */
