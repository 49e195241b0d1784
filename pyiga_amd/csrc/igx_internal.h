// Internal declarations shared by the libigx translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include "igx.h"

namespace igx {

constexpr int MAXP = IGX_MAX_DEGREE + 1;      // max active functions per span
constexpr int MAX_COMP = 4;                   // geometry components incl. NURBS weight

void set_error(const char *fmt, ...);
#define IGX_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            igx::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return IGX_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

// ---------------------------------------------------------------------------------------------
// Device-side views (POD, passed to kernels by value)
struct AxisDev {
    int p, P, N, n, q, G;     // degree, p+1, ndofs, nspans, Gauss pts/span, G = n*q
    int S;                    // number of 1D (i,j) pairs with overlapping support
    const double *nodes;      // [G]
    const double *w;          // [G]
    const double *V;          // [G][P][2]   (value, derivative) of the P active functions
    const double *PI;         // [G][4][P][P] products  PI[t][a][b] = V[b][tu]*V[a][tv], t = tu + 2*tv
                              //              (a: test function i, b: trial function j)
    const int *fa;            // [n]   first active dof of span s
    const int *mslo, *mshi;   // [N]   mesh-span support [mslo, mshi) of dof i
    const int *jlo, *jhi;     // [N]   1D column range of row i
    const int *rp;            // [N+1] exclusive prefix sum of (jhi - jlo): 1D pair index base
    const int *pair_i, *pair_j; // [S]  inverse of the pair index: r -> (i, j)
};

struct PatchDev {
    int dim;
    AxisDev ax[3];
    int r0_lo, r0_hi;         // owned dof planes of axis 0
    int s0_lo, s0_hi;         // resident span range of axis 0
    int g0_lo;                // first resident Gauss index of axis 0 (= s0_lo * q)
    int G0_loc;               // number of resident Gauss planes
    long long npts_loc;       // resident Gauss points = G0_loc * L1 [* L2]
    int b1, b2, L1, L2;       // resident Gauss window of axes 1, 2: first index and extent (whole axes unless the patch is boxed)
    long long nnz_off;        // global indptr[row_lo]
    // IGX_FORM: the terms that are present, in field order; ab = 4 * (jet index of v) + (jet index of u),
    // jet index 0 = value, 1..3 = PARAMETRIC derivative in (x, y, z) order (x = last grid axis)
    // form_par (igx_patch_set_pform): the fields ARE the parametric coefficients (times the Gauss weight); term k differentiates
    // v on the grid axes of mask form_ab[k] >> 3 and u on those of mask form_ab[k] & 7 ("differentiates" = takes slot 1 of the
    // axis' basis table, whose two slots hold the derivative orders chosen with igx_patch_set_basis_orders)
    int form_n;
    int form_ab[16];
    int form_par;
};

// index of Gauss point (g0, g1, g2) in the resident field arrays
__host__ __device__ inline long long field_index(const PatchDev &pd, int g0, int g1, int g2)
{
    const long long l = (long long)(g0 - pd.g0_lo) * pd.L1 + (g1 - pd.b1);
    return pd.dim == 3 ? l * pd.L2 + (g2 - pd.b2) : l;
}

// IGX_FORM coefficients on the resident Gauss slab
struct FormView {
    const double *c;          // [ncoef][npts_loc]
    int slot[16];             // physical coefficient 4*r+s -> row of c, or -1
};

// global CSR row pointer of row (i0,i1,i2); see DESIGN.md "CSR pattern without index arrays"
__host__ __device__ inline long long igx_rowptr3(const int *rp0, const int *rp1, const int *rp2,
                                                 long long S1, long long S2, int c0, int c1,
                                                 int i0, int i1, int i2)
{
    return (long long)rp0[i0] * S1 * S2 + (long long)c0 * ((long long)rp1[i1] * S2 + (long long)c1 * rp2[i2]);
}

// ---------------------------------------------------------------------------------------------
// Host-side state
struct Axis {
    int p = 0, P = 0, N = 0, n = 0, q = 0, G = 0, S = 0;
    bool simple = true;                       // all interior knots have multiplicity 1
    std::vector<double> kv, mesh, nodes, weights;
    std::vector<int> span_knot, fa, mslo, mshi, jlo, jhi, rp, pair_i, pair_j;
    // device
    double *d_kv = nullptr, *d_nodes = nullptr, *d_w = nullptr, *d_V = nullptr, *d_PI = nullptr;
    int *d_ints = nullptr;                    // one allocation: fa | mslo | mshi | jlo | jhi | rp | pair_i | pair_j
    int ord[2] = {0, 1};                      // derivative orders in the two slots of V (and PI)
    AxisDev dev{};
};

struct GeoAxis {                              // geometry basis restricted to the Gauss nodes
    int p = 0, P = 0, N = 0;
    std::vector<double> kv;
    double *d_kv = nullptr;
    double *d_V = nullptr;                    // [G][P][2]
    int *d_fa = nullptr;                      // [G] first active control index at node g
};

} // namespace igx

struct igx_ctx {
    int device = 0;
    int ncu = 0;                              // compute units of THIS context's device (filled by igx_create): launch geometry
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};
};

// Kernel-chain choices of a patch, read from the environment ONCE when the patch is created (igx_patch_create): every
// assembly of the patch takes the same path, whatever happens to the environment afterwards.  None selects a CPU path.
struct igx_knobs {
    int path = 0;                             // IGX_PATH: 0 default (fused in 3D; 2D: one launch for small patches, else stage kernels), 1 fused, 2 unfused, 3 single (2D)
    int geoa = 1;                             // IGX_GEOA=0: separate field and axis-0 sweep kernels
    int geoa_mf = 0;                          // IGX_GEOA=mfma: the FP64 matrix-core form of the axis-0 sweep inside k_geoA at p = 3, 4 (built and
                                              // measured in round 4: 5.08 against 4.50 ms for the vector form at C4 -- DESIGN.md section 3; off by default)
    int final_sel = 0;                        // IGX_FINAL: 0 default, 1 q, 2 valu, 3 mfma (any choice implies the stage kernels)
    int entries_thread = 0;                   // IGX_ENTRIES=thread: one thread per entry (the reference's summation order)
    int poison = 0;                           // IGX_DEBUG_POISON: NaN-fill the CSR values before an assembly and the fields before a field kernel (tests)
    int bf = 0;                               // IGX_BF=2: symmetric 3D forms through k_bf2 + the mirror pass (the chain of rounds 3-4) instead of k_bf3
    int no_twin = 0;                          // IGX_NO_TWIN: no twin patch (repeated knots on the last axis: the stage kernels, as before round 6)
    int no_diag_skip = 0;                     // IGX_NO_DIAG_SKIP: k_geoA writes and k_bf3 reads the K1 slices that diagonal outer pairs duplicate (A/B runs)
    int no_geoa_rot = 0;                      // IGX_NO_GEOA_ROT: the pair window of k_geoA's pair-product sweep moves at every span end, as it does on axes with repeated knots (A/B runs)
    int placement_tries = 1;                  // IGX_PLACEMENT_TRIES=n (opt-in, 3D symmetric forms): the CSR value buffer is the fastest of n
                                              // allocations under the mirror pass, timed once at its first assembly
    int stage_events = -1;                    // IGX_STAGE_EVENTS: events between the kernels of a chain (per-kernel device times in
                                              // igx_last_timing).  A marker costs ~5 us of stream time: default on for 3D patches of
                                              // >= 2^24 Gauss points (kernels of milliseconds), off below and in 2D (kernels of
                                              // 5-40 us), where only the whole interval is timed
};

struct igx_patch;
static inline void stage_event(const igx_patch *pt, int k, hipStream_t st);

struct igx_patch {
    igx_ctx *ctx = nullptr;
    igx_knobs knobs;
    bool basis_default = true;                // every axis' table holds (value, first derivative) (igx_patch_set_basis_orders)
    bool boxed = false;                       // fields only on a span box (igx_patch_desc.box_*): batched entries only
    int dim = 0, nqp = 0;
    igx::Axis ax[3];
    // geometry
    int geo_kind = 0, ncomp = 0;              // ncomp = dim (+1 for NURBS)
    igx::GeoAxis gax[3];
    double *d_ctrl = nullptr;
    double *d_jac = nullptr;                  // IGX_GEO_JACOBIAN: resident slab of the user array
    double *d_formc = nullptr;                // IGX_FORM: physical coefficient fields [n][npts_loc]
    int form_slot[16];                        //   4*r+s -> row of d_formc or -1
    void *form_fn = nullptr;                  // IGX_FORM given as expressions: the generated field kernel (rtc.hip); no d_formc then
    // ... and its PHYSICAL coefficient table as the fast chain reads it (k_geoA<FORM = 2 | 3> evaluates the fields inside the sweep;
    // sumfact.hip: form_table_plan): entry 4 r + s is a constant, an expression (sampled into ftab_arr when the chain first runs),
    // or absent
    struct FormTable {
        bool valid = false, sym = false, blocksym = false;    // sym: P_rs == P_sr for all r, s; blocksym: for r, s >= 1
        int present = 0, is_const = 0;                        // bit masks over 4 r + s
        double cval[16] = {0};
        std::string expr[16];
        int arr_of[16];                                       // index of the entry's array in ftab_arr, or -1
        int narr = 0;
    } ftab;
    double *ftab_arr = nullptr;                               // [narr][npts_loc] sampled non-constant entries (lazily)
    bool ftab_ready = false;
    // Repeated knots on the LAST axis only (round 6): k_bf3 contracts an axis of single knots and sweeps one that may have repeated
    // ones, so such a patch is assembled through its TWIN -- the same patch with mid and last axis exchanged (knot vectors, control
    // net), created with it -- whose k_bf3 stores straight into the CSR layout of this patch (fused3.hip, TR).  twin_kinds: bit per
    // IGX_* kind whose plan on the twin is k_geoA -> k_bf3 (sumfact_twin_kinds); is_twin: this patch is one (its values belong to
    // its owner's layout).
    igx_patch *twin = nullptr;
    int twin_kinds = 0;
    bool is_twin = false;
    double *d_coeff = nullptr;                // IGX_CONVDIFF: scalar coefficient on the resident Gauss slab
    int coef_affine = 0;                      // ... set by igx_patch_set_coeff_affine: k_geoA evaluates it from the geometry map
    bool coeff_sampled = false;               // d_coeff holds the values of the current coefficient (an affine one is sampled only when a kernel that reads the array runs: ensure_coeff)
    double coef_c[4] = {0, 0, 0, 0};
    // slab
    int r0_lo = 0, r0_hi = 0, s0_lo = 0, s0_hi = 0;
    long long row_lo = 0, row_hi = 0, nnz = 0, nnz_off = 0, nrows_total = 0, nelem_owned = 0;
    igx::PatchDev dev{};
    // fields cache
    int fields_kind = -1;
    double *d_fields = nullptr;               // [F][npts_loc]
    size_t fields_cap = 0;
    // CSR
    double *d_data = nullptr;
    int32_t *d_indices = nullptr, *d_indptr = nullptr;
    bool have_pattern = false;
    int values_kind = -1;                     // IGX_* kind d_data holds (igx_assemble / igx_assemble_kron3 done), -1: none or overwritten
                                              // (read by the solver of solve.hip: it refuses values of another kind)
    // sum factorisation workspaces
    bool sumfact_ok = false;
    int *d_pl0 = nullptr;                     // [npairs0][2] processed lower pairs (i0,j0) of axis 0
    int *d_rl0_of = nullptr;                  // [S0] 1D pair index -> compact processed-pair index or -1
    int npairs0 = 0;
    // non-symmetric forms (built on first use): all pairs (i0, j0) of the owned rows i0
    int *d_pl0n = nullptr, *d_stepsn = nullptr;
    int npairs0n = -1;
    // 32-byte line descriptors of the quadrature-lane final kernel (symmetric / non-symmetric pair list)
    int *d_qdesc = nullptr, *d_qdescn = nullptr;
    long long n_qdesc = 0, n_qdescn = 0;
    std::vector<int> h_pl0;                   // host copy of d_pl0 (the line descriptors are built lazily from it)
    bool desc_built = false;
    int *d_ldesc = nullptr;                   // [n_ldesc][4] line descriptors of the final stage
    int n_ldesc = 0;
    int *d_steps = nullptr;                   // flush-step tables of the sweeps (one allocation)
    const int *stepA_ptr = nullptr, *stepA_rec = nullptr, *stepB_ptr = nullptr, *stepB_rec = nullptr;
    float placement_ms_best = 0, placement_ms_worst = 0;   // IGX_PLACEMENT_TRIES: mirror pass on the kept / the slowest candidate
    int placement_tried = 0;
    double *d_geoa_tab = nullptr;             // per-plane records of axis 0 for k_geoA (geoa.hip), built on first use
    int geoa_mf = 0;                          // ... and whether they carry the row tables of the matrix-core sweep
    double *d_geoa_tabn = nullptr;            // the same for the non-symmetric sweep (16-int flush steps), built on first use
    double *d_K1 = nullptr, *d_K2 = nullptr;
    size_t K1_cap = 0, K2_cap = 0;
    // persistent workspaces of the batched-entry and load-vector entry points (grow-only, freed with the patch)
    size_t *d_ws_ij = nullptr; double *d_ws_out = nullptr;
    size_t ws_ij_cap = 0, ws_out_cap = 0;
    long long aca_batch = 65536;              // igx_patch_set_aca_batch
    struct S2DPlan { int valid = 0, ok = 0, R0 = 0, R1 = 0, NG0 = 0, WIN = 0, NCOL = 0; size_t bytes = 0; };
    mutable S2DPlan s2d[2][2];                // tile of the single-launch 2D kernel [mass | stiffness][resident rows | whole patch], worked out once (kern_basis.hip)
    long long aca_requests = 0, aca_entries = 0; int aca_rank = 0;      // igx_fast_assemble_stats
    double *d_lv_f = nullptr, *d_lv_t1 = nullptr, *d_lv_t2 = nullptr, *d_lv_o = nullptr;
    size_t lv_f_cap = 0, lv_t1_cap = 0, lv_t2_cap = 0, lv_o_cap = 0;
    double *d_sp_ws = nullptr;                // axis-0 expansion of igx_patch_eval_spline_d (kern_spline.hip), grow-only
    size_t sp_ws_cap = 0;
    double *d_q_ws = nullptr;                 // partial lines, element sums and totals of igx_patch_quad_sums_d / _error_sums_d (kern_quad.hip), grow-only
    size_t q_ws_cap = 0;
    // igx_patch_residual_sums_d: derivative tables (orders 0, 1, 2: [3][P][G], launch_basis_tables' plain output) of the solution
    // space and of the geometry space per axis, made on first use and kept; the kernels read the order-2 part [P][G]
    double *d_tab2[3] = {nullptr, nullptr, nullptr}, *d_gtab2[3] = {nullptr, nullptr, nullptr};
    bool tab2_ready = false;
    // fused sweep + final stage (fused.hip)
    long long nnz_ext = 0;                    // values of the owned rows + the p0 halo planes above them (mirror sources)
    double *d_zeros = nullptr;                // a row of zeros: input of absent sweep slots
    int *d_triv = nullptr;                    // one-dof outer axis of the 2D case: pl0 {0,0} | rp0 {0,1} | jlo0 {0} | jhi0 {1}
    int *d_tpairs = nullptr;                  // [ntp][2] mirror targets: outer pairs (i0 owned, j0 >= i0)
    int ntp = 0;
    int last_path = 0;                        // kernels of the last sum-factorised assembly: IGX_PATH_* bits
    igx_timing timing{};
};

static inline void stage_event(const igx_patch *pt, int k, hipStream_t st)
{
    if (pt->knobs.stage_events) (void)hipEventRecord(pt->ctx->ev[k], st);
}


// ---------------------------------------------------------------------------------------------
// kernel launchers (defined in the kern_*.hip files)
namespace igx {
// host tables of one axis from its knot vector (igx_api.hip); also the test space of an igx_pair (pair.hip)
int setup_axis(Axis &A, const double *kv, int len, int p, int q, const double *gx, const double *gw);
int launch_basis_tables(hipStream_t st, const double *d_kv, int nk, int p, const double *d_u, size_t nu,
                        int numderiv, double *d_out_nd_p_n /* (nd+1,P,nu) or null */,
                        double *d_V /* [nu][P][2] or null */, int *d_fa /* [nu] or null */,
                        long long *d_spans /* or null */, int o0 = 0, int o1 = 1 /* derivative orders of the two V slots */);
int launch_pi_tables(hipStream_t st, const double *d_V, int G, int P, double *d_PI);
int launch_geo_fields(hipStream_t st, const igx_patch *pt, int kind, double *d_fields);
// which field kernel launch_geo_fields runs: line-wise (LPB lines per block, `lds` bytes of line coefficients) or point-wise.
// One function for the launch and for igx_patch_fields_plan.
struct GeoFieldsPlan { bool lines; int LPB; size_t lds; };
GeoFieldsPlan geo_fields_plan(const igx_patch *pt);
// 2D mass / stiffness in one launch, no intermediates (kern_basis.hip)
bool single2d_supported(const igx_patch *pt, int kind);
bool single2d_wanted(const igx_patch *pt, int kind);                 // the plan's choice (sumfact.hip)
int single2d_plan_query(const igx_patch *pt, int kind, bool whole_patch, int64_t out[9]);   // igx_patch_single2d_plan
long long single2d_blocks(const igx_patch *pt, int kind, int *tile_rows, bool whole_patch);   // launch grid of the single-launch kernel (-1: no tile fits), rows per tile; for the resident rows or as if the patch were whole
int launch_single2d(hipStream_t st, igx_patch *pt, int kind, double *d_data);
int launch_grid_geo(hipStream_t st, int dim, int ncomp_total, bool nurbs, const GeoAxis gax[3],
                    const int G[3], const double *d_ctrl, double *d_jac, double *d_eval);
int launch_fields_dump(hipStream_t st, const igx_patch *pt);
int launch_coeff_affine(hipStream_t st, const igx_patch *pt, const double c[4], double *d_coeff);
// Kronecker expansion of a separable geometry (kron.hip)
int launch_kron3(hipStream_t st, igx_patch *p3, const double *d_a0, const double *d_b0, int C0, const double *d_A2, const double *d_B2);
// run-time compiled coefficient expressions (rtc.hip)
int launch_coeff_expr(hipStream_t st, igx_patch *pt, const char *expr, double *d_coeff, int *cache_hit, bool parametric = false /* x, y, z = parametric coordinates */);
int lv12_expr_applicable(const igx_patch *pt, int parametric);   // IGX_OK | IGX_ERR_UNSUPPORTED (shape) | IGX_ERR_NORTC (no libhiprtc)
int rtc_compile_expr(const char *expr, const char *arch, char *path_out, int path_len, int *cache_hit);
int launch_form_exprs(hipStream_t st, igx_patch *pt, int n_expr, const char *const *expr, double *d_out /* [n_expr][npts_loc] */, int *cache_hit);
int rtc_compile_form(int n_expr, const char *const *expr, const char *arch, char *path_out, int path_len, int *cache_hit);
// field kernel of a form given as expressions (geometry + coefficients + jet transformation in one generated kernel)
int rtc_form_fields_function(igx_patch *pt, const char *const expr[16], int nterms, const int *form_ab, void **fn_out, int *cache_hit, bool parametric = false);
int launch_form_fields(hipStream_t st, const igx_patch *pt, void *fn, double *d_fields);
bool form_fields_applicable(const igx_patch *pt);
// 3D load vector with the function inside the first two contractions (rtc.hip) + helpers of kern_vector.hip
int launch_lv12_expr(hipStream_t st, igx_patch *pt, const char *expr, int parametric, const double *d_W, double *d_t2, int *cache_hit);
int rtc_compile_lv12(int P, int npass, int parametric, const char *expr, const char *arch, char *path_out, int path_len, int *cache_hit);
bool lv12_shape(const igx_patch *pt, int *clen_out, int *nch_out, size_t *lds_out);
int launch_lv_axis0(hipStream_t st, const igx_patch *pt, const double *d_t2, double *d_out, int deriv0, int accumulate);
int form_terms(int dim, const char *const expr[16], int form_ab[16]);
int rtc_compile_form_fields(int dim, int ncomp, const char *const expr[16], const char *arch, char *path_out, int path_len, int *cache_hit);
int launch_pattern(hipStream_t st, const igx_patch *pt, int32_t *d_indptr, int32_t *d_indices);
int launch_entries_list(hipStream_t st, const igx_patch *pt, int kind, const size_t *d_ij, size_t M, double *d_out);
// boxes of the reordered tensor X[r0][r1][r2] (r_k = index of a 1D pair (i_k, j_k) with overlapping supports): the entries
// lo[b][k] <= r_k < lo[b][k] + len[b][k] of every box, box after box, lexicographic inside a box
struct PairBoxes { int n; int lo[8][3], len[8][3]; long long off[9]; };
int launch_box_pairs(hipStream_t st, const igx_patch *pt, const PairBoxes &B, size_t *d_ij);
int entries_pair_boxes(igx_patch *pt, int kind, const PairBoxes &B, double *out_host);   // (igx_api.hip: index pairs built on the device)
int launch_entries_csr(hipStream_t st, const igx_patch *pt, int kind, double *d_data);
int launch_load_vector(hipStream_t st, const igx_patch *pt, const double *d_f, const double *d_W, double *d_out,
                       double *d_t1, double *d_t2, int deriv_axis = -1, int accumulate = 0, int *n_launches = nullptr /* 2: k_lv12 + axis 0, else one per axis */);
// a spline of the patch's space from a device dof vector at the resident Gauss points (kern_spline.hip)
size_t spline_eval_workspace(const igx_patch *pt, int want_grad);
int launch_spline_eval(hipStream_t st, const igx_patch *pt, const double *d_coeffs, int want_grad, double *const d_out[4], double *d_ws);
size_t vspline_eval_workspace(const igx_patch *pt, int nc, int want_grad);
int launch_vspline_eval(hipStream_t st, const igx_patch *pt, int nc, const double *d_coeffs, int want_grad, double *const d_out[12], double *d_ws);
int launch_spline_axis0(hipStream_t st, const igx_patch *pt, const double *d_coeffs, int want_grad, double *d_ws, const double **t0, const double **t1);
// sums of W f_k and error sums of a spline over a whole patch, total and per element, in a fixed order (kern_quad.hip)
size_t quad_workspace(const igx_patch *pt, int nk);
int launch_quad_sums(hipStream_t st, const igx_patch *pt, int nf, const double *const *d_f, const double *d_W, double *d_elem, double *d_ws,
                     double **d_tot, int *n_launches);
int launch_error_sums(hipStream_t st, const igx_patch *pt, const double *d_coeffs, int want_grad, const double *const d_exact[4], const double *d_W,
                      double *d_elem, double *d_sp_ws, double *d_ws, double **d_tot, int *n_launches);
// element residual sums  sum W (f + Lap u_h)^2, sum W  of a spline (kern_quad.hip: k_res12); the axis-0 pre-pass with the second
// derivative (kern_spline.hip)
int launch_spline_axis0_d2(hipStream_t st, const igx_patch *pt, const double *d_coeffs, const double *d_d2, double *d_ws);
size_t residual_spline_workspace(const igx_patch *pt);
int residual_tables(hipStream_t st, igx_patch *pt);
int launch_residual_sums(hipStream_t st, const igx_patch *pt, const double *d_coeffs, const double *d_f, const double *d_W,
                         double *d_elem, double *d_sp_ws, double *d_ws, double **d_tot, int *n_launches);
// coefficient expressions that also read device arrays f0 .. f{m-1} at the thread's point (rtc.hip)
int launch_form_exprs_inputs(hipStream_t st, igx_patch *pt, int n_expr, const char *const *expr, int m, const double *const *d_in, double *d_out, int *cache_hit);
int rtc_compile_form_inputs(int n_expr, const char *const *expr, int m, const char *arch, char *path_out, int path_len, int *cache_hit);
inline int igx_num_fields(int dim, int kind, int form_n = 0)
{
    return kind == IGX_MASS ? 1 : (kind == IGX_CONVDIFF ? 9 : (kind == IGX_FORM ? form_n : dim * (dim + 1) / 2));
}
constexpr size_t IGX_DUMP_PAD = 1024 * 16 + 16;   // doubles behind the CSR values: 1024 dump lines of the final stage
inline bool igx_kind_symmetric(int kind) { return kind != IGX_CONVDIFF && kind != IGX_FORM; }
// fused sweep + final stage and mirror pass (fused.hip)
struct BFInputs {
    int pad_stiff3 = 0;                       // treat the slot set as the full first-order set (absent slots read the zero row): general forms
    int tr = 0;                               // the patch is the axis-exchanged twin of the caller's (igx_patch::twin): k_bf3 stores to the caller's CSR layout
    const Axis *mid, *last;                   // swept axis, last (contiguous) axis
    int slot_n[4][4];                         // [last-axis type y][mid-axis type t1]: number of input arrays (<= 2)
    const double *slot_ptr[4][4][2];          // their device pointers: array[slice][g_mid - gmid_lo][g_last]
    long long slice_stride;                   // doubles between slices (outer pairs)
    const double *zeros;                      // >= G_last zeros
    int gmid_lo;
    const int *pl0;                           // [npairs][2] outer pairs (device)
    int npairs;
    const int *rp0, *jlo0, *jhi0;             // outer axis tables (device)
    int sym, mid_lo, mid_hi;
    int span_hi;                              // resident spans of the mid axis end here
    // k_bf3, 3D stiffness (Plan::diag_skip): on a DIAGONAL outer pair the array of slot (y, t1) is read from diag_ptr[y][t1] -- the
    // other member of its couple where k_geoA leaves the slot's own slice unwritten -- and (diag_tr) the role of last-axis type 2
    // loads nothing: its lines are the transposed window of the role of type 1
    int diag_skip = 0, diag_tr = 0;
    const double *diag_ptr[4][4];
};
struct MirrorInputs {
    const Axis *mid, *last;
    const int *rp0, *jlo0, *jhi0;
    const int *tpairs;
    int ntp;
    int i1_lo, i1_hi;                         // target rows of the mid axis
};
int fused_supported(const BFInputs &in);
// 32-bit buffer offsets of k_bf2 / k_mirror2 (fused.hip): row block of an outer row and a K1 slice below 2^31 bytes
bool fused_offsets_fit(long long c0max, long long S_mid, long long S_last, long long G_mid, long long G_last);
// host arithmetic of launch_bf (igx_fused_rows_per_tile, igx_fused_chunk_plan): rows of the last axis per tile of k_bf2<P, ., mask, na>;
// {mrows, nmchunks, main_blocks, tail_k, tail_mrows} of bf2_choose_chunks
int fused2_rows_per_tile(int P, int mask, int na);
void fused2_chunk_plan(int npairs, int ntiles, int mid_rows, long long slots, int P, int out[5]);
int launch_bf(hipStream_t st, const igx_patch *pt, const BFInputs &in, double *d_data);
int launch_mirror(hipStream_t st, const igx_patch *pt, const MirrorInputs &in, double *d_data);
// k_bf3 (fused3.hip): the fused stage of the symmetric forms that writes both triangles itself (no mirror pass)
bool fused3_supported(const BFInputs &in);
bool fused3_offsets_fit(int dim, int p0, int p1, int p2, long long S_mid, long long S_last, long long N_last);
bool fused3_degrees(int P1, int P2, int Q, bool sym3d, bool mid_simple);
bool fused3_tr_fits(int p0, int p1, int p2, long long S_mid, long long S_last);
int launch_bf3(hipStream_t st, const igx_patch *pt, const BFInputs &in, double *d_data);
// fused geometry + stage A (geoa.hip)
bool geoA_supported(const igx_patch *pt, int kind, int nslots);
// the axis-0 sweep this patch takes forms V_a[tv] V_b[tu] as ONE product per (plane, pair): on a pair a = b the arrays of the
// axis-0 types 1 and 2 over the same field are then the same bits (the pair-product sweep of k_geoA: p <= 4, vector form)
bool geoA_diag_types_commute(const igx_patch *pt);
// table of a general first-order form for k_geoA (FORM = 2 | 3): see GeoAArgs (geoa.hip)
struct GeoAForm {
    int sym;                                  // symmetric table: lower pairs of axis 0, symmetric flush
    double pc[16];
    const double *pa[16];
    int pmask;
    int fslot[16];
    int nsrc[8], sfield[8][4], stype[8][4];
};
int launch_geoA(hipStream_t st, igx_patch *pt, int kind, int nslots, const int *slot_field, const int *slot_type,
                double *const *slot_out, long long slice_stride, int chunk_len, int nchunks, const int *slot_xfield = nullptr, const int *slot_xtype = nullptr,
                const GeoAForm *form = nullptr, unsigned nodiag_mask = 0);
bool geoA_form_supported(const igx_patch *pt);

// The kernel chain of one sum-factorised assembly: sumfact_plan decides all of it from the patch, its knobs and the kind (no HIP
// calls), sumfact_assemble runs it.  The chains:
//   FORM_TABLE  k_geoA<FORM = 2 | 3> -> k_bf3                   a coefficient table (form_table_plan)
//   SINGLE2D    k_single2d                                      small 2D patches
//   FUSED2D     the field arrays -> k_bf3, or k_bf2 + k_mirror2  (IGX_PATH=fused in 2D)
//   STAGES      k_geoA or k_stageA -> k_bf3, or k_bf2 (+ k_mirror2), or k_stageB / k_combine -> k_final_mfma, k_final_q or k_final
// twin: the plan is that of pt->twin (repeated knots on the last axis only), whose values land in the patch's layout.
struct Term;                                  // sumfact_stages.h
struct XA { int t0, f, slot, key, xt0, xf, alias; };   // stage-A array: axis-0 type, field (+ second source of a merged slot)
struct FormPlan {
    bool ok = false, sym = false;
    GeoAForm g;
    int narr = 0;
    int slot_arr[4][4];                       // (last-axis type y, mid-axis type t1) -> K1 array, or -1
    bool mass_only = false;
};
struct Plan {
    enum Chain { FORM_TABLE, SINGLE2D, FUSED2D, STAGES };
    enum Fused { NO_FUSED, BF3, BF2 };
    enum Final { FINAL_VALU, FINAL_Q, FINAL_MFMA };
    int kind = 0;
    bool sym = false, twin = false;
    Chain chain = STAGES;
    bool needs_fields = false;                // the chain reads the field arrays (igx_assemble computes them first)
    bool one_launch = false;                  // no stage events (k_single2d)
    // K1 arrays of the stage chain (the field arrays in FUSED2D): terms of the form, their stage-A arrays X, term -> X.  merged
    // (non-symmetric 3D forms into the fused stage): one array per fused-stage slot, an alias shares an earlier slot's array
    std::vector<Term> terms;
    std::vector<XA> X;
    std::vector<int> term_x;
    bool merged = false;
    int nX = 0;
    bool geoA = false;                        // stage 0: k_geoA, else k_stageA
    Fused fused = NO_FUSED;
    int slot_n[4][4] = {}, slot_arr[4][4][2]; // fused-stage inputs per (last-axis type, mid-axis type): count, array index
    // 3D stiffness through k_geoA -> k_bf3: the arrays of a couple -- same field, axis-0 types 1 and 2 -- are the same bits on a
    // diagonal outer pair.  diag_skip: k_geoA does not write those slices of the arrays in nodiag_mask (the members of type 1) and
    // k_bf3 reads slot (y, t1) of a diagonal block from array diag_arr[y][t1]; diag_tr: with that, the inputs of the role of
    // last-axis type 2 are those of type 1 with the mid-axis types transposed
    bool diag_skip = false, diag_tr = false;
    unsigned nodiag_mask = 0;
    int diag_arr[4][4] = {};
    Final fin = FINAL_VALU;
    int mfma_nch = 0;                         // k_final_mfma: 8-point chunks of the Gauss window
    FormPlan form;
    Plan();                                   // (out of line: Term is complete in sumfact.hip)
    ~Plan();
};
void sumfact_plan(const igx_patch *pt, int kind, Plan &pl);
int sumfact_twin_kinds(const igx_patch *tw);                    // IGX_* kinds (bit mask) the fast chain of an axis-exchanged twin serves
// device time of the mirror pass of this plan on `buf` (access pattern only: the values are whatever the buffer holds);
// < 0 when the plan has no such pass
float sumfact_probe_mirror(igx_patch *pt, const Plan &pl, double *buf);
int sumfact_supported(const igx_patch *pt);
int sumfact_prepare(igx_patch *pt);
int sumfact_supports_kind(const igx_patch *pt, int kind);
int sumfact_assemble(igx_patch *pt, const Plan &pl, double *d_data);
} // namespace igx

// ---------------------------------------------------------------------------------------------
// multipatch handle (multipatch.hip); also read by the multipatch solver (solve.hip)
namespace igx {
struct RowInfo {                             // per local row of a patch: the scatter plan (16 bytes)
    int32_t kstart, len, base, mode;         // base: delta (DIRECT) or offset of the row in the compacted position array
};
enum { MODE_DIRECT = 0, MODE_STORE = 1, MODE_RMW = 2, MODE_ATOMIC = 3 };   // RowInfo::mode: how the row's values reach the sums
} // namespace igx

struct igx_multipatch {
    igx_ctx *ctx = nullptr;
    int np = 0;
    long long nglobal = 0, nnz = 0;
    bool injective = true;
    long long zero_from = 0;                   // igx_multipatch_zero clears values [zero_from, nnz): the rows more than one local row reaches
    long long vzero_from = 0;                  // ... and vector entries [vzero_from, nglobal)
    unsigned long long generation = 0;         // bumped by igx_multipatch_zero: a solver made over older sums refuses to run
    unsigned long long scattered = ~0ULL;      // the generation whose sums last received a patch's values (none yet: no generation)
    int32_t *d_indptr = nullptr, *d_indices = nullptr, *d_contrib = nullptr;
    double *d_vals = nullptr, *d_vec = nullptr, *d_stage = nullptr;
    size_t stage_len = 0;
    long long counts[4] = {0, 0, 0, 0};        // local entries per scatter class
    int max_row = 0;                           // longest global row (entries)
    struct Patch {
        int n = 0;
        int dim = 0, N[3] = {1, 1, 1};         // tensor-product shape of the patch's dofs
        long long nnz = 0;
        int32_t *d_l2g = nullptr;
        igx::RowInfo *d_info = nullptr;
        int32_t *d_cpos = nullptr;
        // per-axis tables of the patch's value layout (igx_multipatch_add_face): host copies and one device allocation
        // jlo | jhi | rp per axis, axis k at d_tab + tab_pos[k][0 .. 2]
        std::vector<int> jlo[3], jhi[3], rp[3];
        int p[3] = {0, 0, 0};
        int *d_tab = nullptr;
        size_t tab_pos[3][3] = {};
        unsigned long long scattered = ~0ULL;  // the generation of the sums that last received this patch's values
    };
    std::vector<Patch> pp;
};
