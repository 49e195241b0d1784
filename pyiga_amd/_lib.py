"""ctypes binding of libigx (include/igx.h).  Thin: argument marshalling only.

There is no CPU fallback: if the shared library is missing, or no MI355X is
visible when a context is requested, this raises.
"""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# IGX_LIB selects another build of the same library (kernel ablation builds); never a fallback
LIB_PATH = os.environ.get('IGX_LIB') or os.path.join(_HERE, 'libigx.so')

IGX_MASS, IGX_STIFFNESS, IGX_CONVDIFF, IGX_FORM = 0, 1, 2, 3
IGX_GEO_BSPLINE, IGX_GEO_NURBS, IGX_GEO_JACOBIAN = 0, 1, 2
IGX_ALGO_AUTO, IGX_ALGO_ENTRYWISE, IGX_ALGO_SUMFACT = 0, 1, 2
ALGOS = {'auto': IGX_ALGO_AUTO, 'entrywise': IGX_ALGO_ENTRYWISE, 'sumfact': IGX_ALGO_SUMFACT}
KINDS = {'mass': IGX_MASS, 'stiffness': IGX_STIFFNESS, 'convdiff': IGX_CONVDIFF, 'form': IGX_FORM}

_dp = C.POINTER(C.c_double)


class PatchDesc(C.Structure):
    _fields_ = [
        ('dim', C.c_int32), ('p', C.c_int32 * 3), ('kv_len', C.c_int32 * 3), ('kv', _dp * 3),
        ('geo_kind', C.c_int32), ('geo_p', C.c_int32 * 3), ('geo_kv_len', C.c_int32 * 3), ('geo_kv', _dp * 3),
        ('ctrl', _dp), ('jac', _dp),
        ('nqp', C.c_int32), ('gauss_x', _dp), ('gauss_w', _dp),
        ('row0_lo', C.c_int32), ('row0_hi', C.c_int32),
        ('box_lo', C.c_int32 * 3), ('box_hi', C.c_int32 * 3),
    ]


class PatchInfo(C.Structure):
    _fields_ = [
        ('dim', C.c_int32), ('nqp', C.c_int32),
        ('ndofs', C.c_int32 * 3), ('nspans', C.c_int32 * 3), ('ngauss', C.c_int32 * 3),
        ('nrows_total', C.c_int64), ('row_lo', C.c_int64), ('row_hi', C.c_int64),
        ('nnz', C.c_int64), ('nnz_offset', C.c_int64), ('nelem_owned', C.c_int64),
        ('sumfact_ok', C.c_int32), ('reserved', C.c_int32),
    ]


class PairInfo(C.Structure):
    _fields_ = [
        ('dim', C.c_int32), ('reserved', C.c_int32), ('ndofs_trial', C.c_int32 * 3), ('ndofs_test', C.c_int32 * 3),
        ('nrows', C.c_int64), ('ncols', C.c_int64), ('nnz', C.c_int64),
    ]


class MultipatchInfo(C.Structure):
    _fields_ = [
        ('npatches', C.c_int32), ('injective', C.c_int32), ('nrows', C.c_int64), ('nnz', C.c_int64),
        ('entries', C.c_int64 * 4), ('zero_from', C.c_int64),
    ]


class Timing(C.Structure):
    _fields_ = [
        ('total_ms', C.c_float), ('fields_ms', C.c_float), ('stage0_ms', C.c_float),
        ('stage1_ms', C.c_float), ('final_ms', C.c_float), ('entry_ms', C.c_float),
        ('algo_used', C.c_int32), ('n_launches', C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


IGX_PRECOND_NONE, IGX_PRECOND_JACOBI, IGX_PRECOND_KRON, IGX_PRECOND_SCHWARZ, IGX_PRECOND_MG = 0, 1, 2, 3, 4
IGX_KRON_SUM, IGX_KRON_PRODUCT = 1, 2
PRECONDS = {None: IGX_PRECOND_NONE, 'none': IGX_PRECOND_NONE, 'jacobi': IGX_PRECOND_JACOBI, 'kron': IGX_PRECOND_KRON}
MP_PRECONDS = {None: IGX_PRECOND_NONE, 'none': IGX_PRECOND_NONE, 'jacobi': IGX_PRECOND_JACOBI, 'schwarz': IGX_PRECOND_SCHWARZ,
               'mg': IGX_PRECOND_MG}
MPVEC_PRECONDS = {None: IGX_PRECOND_NONE, 'none': IGX_PRECOND_NONE, 'jacobi': IGX_PRECOND_JACOBI, 'schwarz': IGX_PRECOND_SCHWARZ,
                  'mg': IGX_PRECOND_MG}
IGX_METHOD_CG, IGX_METHOD_BICGSTAB, IGX_METHOD_MINRES = 0, 1, 2
METHODS = {'cg': IGX_METHOD_CG, 'bicgstab': IGX_METHOD_BICGSTAB}
SADDLE_METHODS = dict(METHODS, minres=IGX_METHOD_MINRES)      # (MINRES: saddle-point solvers, and only they)
IGX_BREAKDOWN_RHO, IGX_BREAKDOWN_ALPHA, IGX_BREAKDOWN_OMEGA, IGX_BREAKDOWN_NONFINITE, IGX_BREAKDOWN_INDEFINITE_PRECOND = 1, 2, 3, 4, 5
BREAKDOWNS = {0: None, IGX_BREAKDOWN_RHO: 'rho', IGX_BREAKDOWN_ALPHA: 'alpha', IGX_BREAKDOWN_OMEGA: 'omega',
              IGX_BREAKDOWN_NONFINITE: 'nonfinite', IGX_BREAKDOWN_INDEFINITE_PRECOND: 'indefinite_precond'}


class SolveInfo(C.Structure):
    _fields_ = [
        ('iterations', C.c_int32), ('converged', C.c_int32), ('relres', C.c_double), ('n_free', C.c_int64),
        ('spmv_ms', C.c_float), ('precond_ms', C.c_float), ('vector_ms', C.c_float), ('total_ms', C.c_float),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MgInfo(C.Structure):
    _fields_ = [
        ('nrows', C.c_int64), ('nfree', C.c_int64), ('nnz', C.c_int64), ('ncolours', C.c_int32), ('one_block', C.c_int32),
        ('smooth_steps', C.c_int32), ('dense_inverse', C.c_int32), ('has_coarse', C.c_int32), ('reserved', C.c_int32),
    ]


IGX_MG_MAX_LEVELS = 16


class MgProfile(C.Structure):
    _fields_ = [
        ('levels', C.c_int32), ('launches', C.c_int32), ('total_ms', C.c_float), ('coarse_ms', C.c_float), ('vector_ms', C.c_float),
        ('reserved', C.c_float), ('smooth_ms', C.c_float * IGX_MG_MAX_LEVELS), ('residual_ms', C.c_float * IGX_MG_MAX_LEVELS),
        ('transfer_ms', C.c_float * IGX_MG_MAX_LEVELS),
    ]


IGX_DIRK_MAX_STAGES = 6
IGX_ROLE_MASS, IGX_ROLE_OPERATOR = 0, 1


class DirkInfo(C.Structure):
    _fields_ = [
        ('steps', C.c_int64), ('converged', C.c_int32), ('nsaved', C.c_int32), ('iterations', C.c_int64),
        ('max_stage_iterations', C.c_int32), ('reserved', C.c_int32),
        ('axpby_ms', C.c_float), ('spmv_ms', C.c_float), ('combine_ms', C.c_float), ('solve_ms', C.c_float),
        ('total_ms', C.c_float), ('reserved2', C.c_float),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith('reserved')}


IGX_STEPPER_DIRK, IGX_STEPPER_ROSENBROCK = 0, 1
IGX_STEP_STATE, IGX_STEP_CANDIDATE = 0, 1
COMB_MAX = 8                    # vectors of one k_dirk_rhs / k_err_norm pass (csrc/solve_step.hip)


class StepInfo(C.Structure):
    _fields_ = [
        ('r', C.c_double), ('converged', C.c_int32), ('reformed', C.c_int32), ('has_estimate', C.c_int32),
        ('mass_iterations', C.c_int32), ('stage_iterations', C.c_int32 * IGX_DIRK_MAX_STAGES), ('n_free', C.c_int64),
        ('axpby_ms', C.c_float), ('spmv_ms', C.c_float), ('combine_ms', C.c_float), ('solve_ms', C.c_float),
        ('mass_ms', C.c_float), ('err_ms', C.c_float), ('total_ms', C.c_float), ('reserved', C.c_float),
    ]


IGX_EIG_BLOCKS = {'X': 0, 'KX': 1, 'MX': 2, 'W': 3, 'KW': 4, 'MW': 5, 'P': 6, 'KP': 7, 'MP': 8, 'R': 9}


class EigInfo(C.Structure):
    _fields_ = [
        ('m', C.c_int32), ('mb', C.c_int32), ('products', C.c_int32), ('grams', C.c_int32), ('combines', C.c_int32),
        ('residuals', C.c_int32), ('preconds', C.c_int32), ('reserved', C.c_int32), ('n_free', C.c_int64),
        ('products_ms', C.c_float), ('gram_ms', C.c_float), ('combine_ms', C.c_float), ('residual_ms', C.c_float),
        ('precond_ms', C.c_float), ('reserved2', C.c_float),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith('reserved')}


class HierAxis(C.Structure):
    _fields_ = [
        ('d_clo', C.c_void_p), ('d_ccnt', C.c_void_p), ('d_w', C.c_void_p), ('d_first', C.c_void_p), ('d_cnt', C.c_void_p),
        ('wmax', C.c_int32), ('n_coarse', C.c_int32), ('n_fine', C.c_int32), ('box_lo', C.c_int32), ('box_n', C.c_int32),
        ('reserved', C.c_int32),
    ]


class HierBlock(C.Structure):
    _fields_ = [
        ('dim', C.c_int32), ('symmetric', C.c_int32), ('ax', HierAxis * 3),
        ('d_slot', C.c_void_p), ('d_rowptr', C.c_void_p), ('d_entries', C.c_void_p), ('n_entries', C.c_int64),
        ('d_ia', C.c_void_p), ('d_ib', C.c_void_p), ('d_pos', C.c_void_p), ('d_pos2', C.c_void_p), ('n_items', C.c_int64),
        ('group', C.c_int32), ('max_blocks', C.c_int32),
    ]


IGX_HMG_MAX_LEVELS = 16
HMG_SMOOTHERS = {'gs': 0, 'forward_gs': 1, 'backward_gs': 2, 'symmetric_gs': 3}
HMG_METHODS = {'iterate': 0, 'cg': 1}


class HmgInfo(C.Structure):
    _fields_ = [('iterations', C.c_int32), ('converged', C.c_int32), ('ratio', C.c_double), ('n_free', C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class HmgProfile(C.Structure):
    _fields_ = [
        ('levels', C.c_int32), ('launches', C.c_int32), ('total_ms', C.c_float), ('coarse_ms', C.c_float),
        ('smooth_ms', C.c_float * IGX_HMG_MAX_LEVELS), ('residual_ms', C.c_float * IGX_HMG_MAX_LEVELS),
        ('transfer_ms', C.c_float * IGX_HMG_MAX_LEVELS),
    ]


class HmgLevel(C.Structure):
    _fields_ = [
        ('nrows', C.c_int64), ('nnz', C.c_int64), ('nsmooth', C.c_int64), ('ncolours', C.c_int32), ('one_block', C.c_int32),
        ('group_width', C.c_int32), ('reserved', C.c_int32),
    ]


class KronDesc(C.Structure):
    _fields_ = [
        ('dim', C.c_int32), ('m', C.c_int32 * 3), ('n', C.c_int32 * 3), ('d_B', C.c_void_p * 3),
        ('batch', C.c_int64), ('x_off', C.c_int64), ('x_stride', C.c_int64 * 4), ('y_off', C.c_int64), ('y_stride', C.c_int64 * 4),
        ('lam_mode', C.c_int32), ('reserved', C.c_int32), ('d_lam', C.c_void_p * 3),
    ]


# every symbol include/igx.h declares: (name, restype, argtypes)
SYMBOLS = [
    ('igx_version', C.c_int, []),
    ('igx_last_error', C.c_char_p, []),
    ('igx_create', C.c_void_p, [C.c_int]),
    ('igx_destroy', None, [C.c_void_p]),
    ('igx_sync', C.c_int, [C.c_void_p]),
    ('igx_stream', C.c_void_p, [C.c_void_p]),
    ('igx_active_deriv', C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, _dp, C.c_size_t, C.c_int, _dp]),
    ('igx_find_spans', C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, _dp, C.c_size_t, C.POINTER(C.c_int64)]),
    ('igx_grid_jacobian', C.c_int, [C.c_void_p, C.POINTER(PatchDesc), C.c_int, _dp * 3, C.c_int32 * 3, _dp, _dp]),
    ('igx_patch_create', C.c_void_p, [C.c_void_p, C.POINTER(PatchDesc)]),
    ('igx_patch_destroy', None, [C.c_void_p]),
    ('igx_patch_get_info', C.c_int, [C.c_void_p, C.POINTER(PatchInfo)]),
    ('igx_patch_set_coeff', C.c_int, [C.c_void_p, _dp]),
    ('igx_patch_set_form', C.c_int, [C.c_void_p, _dp * 16]),
    ('igx_patch_eval_expr_d', C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    ('igx_patch_set_form_expr', C.c_int, [C.c_void_p, C.c_char_p * 16, C.POINTER(C.c_int)]),
    ('igx_rtc_compile_form', C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    ('igx_patch_form_generated', C.c_int, [C.c_void_p]),
    ('igx_load_vector_expr', C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    ('igx_rtc_compile_load_vector', C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    ('igx_rtc_compile_form_fields', C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    ('igx_patch_set_pform', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(_dp)]),
    ('igx_patch_set_basis_orders', C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ('igx_patch_gauss', C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    ('igx_pattern', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ('igx_assemble', C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp]),
    ('igx_last_timing', C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    ('igx_d_csr_data', C.c_void_p, [C.c_void_p]),
    ('igx_d_csr_indices', C.c_void_p, [C.c_void_p]),
    ('igx_d_csr_indptr', C.c_void_p, [C.c_void_p]),
    ('igx_entries', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.c_size_t, _dp]),
    ('igx_fields', C.c_int, [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int64)]),
    ('igx_fused_stage_fits', C.c_int, [C.c_int64] * 5),
    ('igx_fused_rows_per_tile', C.c_int, [C.c_int] * 3),
    ('igx_fused_chunk_plan', C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int)]),
    ('igx_patch_fields_plan', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    ('igx_patch_single2d_plan', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    ('igx_assemble_kron3', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _dp, _dp, _dp]),
    ('igx_patch_set_coeff_expr', C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    ('igx_rtc_compile', C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    ('igx_patch_placement', C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ('igx_load_vector', C.c_int, [C.c_void_p, _dp, _dp]),
    ('igx_load_vector_jet', C.c_int, [C.c_void_p, _dp * 4, _dp]),
    ('igx_load_vector_jet_expr', C.c_int, [C.c_void_p, C.c_char_p * 4, _dp, C.POINTER(C.c_int)]),
    ('igx_entries_d', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    ('igx_load_vector_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ('igx_fast_assemble', C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    ('igx_patch_set_aca_batch', C.c_int, [C.c_void_p, C.c_longlong]),
    ('igx_fast_assemble_stats', C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    ('igx_patch_set_coeff_affine', C.c_int, [C.c_void_p, C.c_double * 4]),
    ('igx_patch_set_form_d', C.c_int, [C.c_void_p, C.c_void_p * 16]),
    ('igx_patch_last_path', C.c_int, [C.c_void_p]),
    ('igx_patch_eval_spline_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p * 4]),
    ('igx_patch_quad_sums_d', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, _dp]),
    ('igx_patch_error_sums_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p * 4, C.c_void_p, _dp]),
    ('igx_patch_residual_sums_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _dp]),
    ('igx_patch_eval_exprs_inputs_d', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_int)]),
    ('igx_rtc_compile_exprs_inputs', C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    ('igx_load_vector_jet_d', C.c_int, [C.c_void_p, C.c_void_p * 4, C.c_void_p]),
    ('igx_patch_gauss_slab', C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ('igx_hier_contract_d', C.c_int, [C.c_void_p, C.POINTER(HierBlock), C.c_void_p, C.c_int64, C.POINTER(C.c_float)]),
    ('igx_hier_gather_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    ('igx_dev_alloc', C.c_void_p, [C.c_void_p, C.c_size_t]),
    ('igx_dev_free', None, [C.c_void_p, C.c_void_p]),
    ('igx_dev_upload', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ('igx_dev_download', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    ('igx_multipatch_create', C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_int32)), C.c_int64]),
    ('igx_multipatch_destroy', None, [C.c_void_p]),
    ('igx_multipatch_get_info', C.c_int, [C.c_void_p, C.POINTER(MultipatchInfo)]),
    ('igx_multipatch_pattern', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ('igx_multipatch_zero', C.c_int, [C.c_void_p]),
    ('igx_multipatch_scatter_patch', C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    ('igx_multipatch_scatter_host', C.c_int, [C.c_void_p, C.c_int, _dp]),
    ('igx_multipatch_scatter_vector', C.c_int, [C.c_void_p, C.c_int, _dp]),
    ('igx_multipatch_download', C.c_int, [C.c_void_p, _dp, _dp]),
    ('igx_multipatch_values_d', C.c_int, [C.c_void_p, C.c_void_p]),
    ('igx_patch_add_face', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ('igx_patch_add_face_host', C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int64]),
    ('igx_multipatch_add_face', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ('igx_multipatch_add_face_host', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, C.c_int64]),
    ('igx_solver_create', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_void_p)]),
    ('igx_solver_create_general', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_void_p)]),
    ('igx_solver_set_method', C.c_int, [C.c_void_p, C.c_int]),
    ('igx_solver_last_breakdown', C.c_int, [C.c_void_p]),
    ('igx_solver_create_multipatch', C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_void_p)]),
    ('igx_solver_create_block', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_void_p)]),
    ('igx_solver_take_block', C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ('igx_solver_set_block_kron', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_dp), C.POINTER(_dp), C.c_int]),
    ('igx_solver_create_multipatch_block', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_void_p)]),
    ('igx_solver_take_multipatch_block', C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ('igx_solver_download_multipatch_block', C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp]),
    ('igx_solver_set_block_schwarz', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_dp), C.POINTER(_dp), C.c_int]),
    ('igx_solver_destroy', None, [C.c_void_p]),
    ('igx_solver_set_precond', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_dp), C.POINTER(_dp), C.c_int]),
    ('igx_solver_set_schwarz', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_dp), C.POINTER(_dp), C.c_int]),
    ('igx_csr_colouring', C.c_int, [C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32)]),
    ('igx_solver_set_mg_smoother', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int64]),
    ('igx_solver_set_mg_coarse', C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_dp), _dp]),
    ('igx_solver_set_mg_inverse', C.c_int, [C.c_void_p, _dp, C.c_int64]),
    ('igx_solver_set_block_mg_smoother', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    ('igx_solver_set_block_mg_coarse', C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_dp), _dp]),
    ('igx_solver_set_block_mg_inverse', C.c_int, [C.c_void_p, _dp, C.c_int64]),
    ('igx_solver_mg_info', C.c_int, [C.c_void_p, C.c_int, C.POINTER(MgInfo)]),
    ('igx_solver_mg_colours', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ('igx_solver_mg_profile_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(MgProfile)]),
    ('igx_solver_mg_relax_d', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ('igx_solver_mg_prolong_d', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ('igx_solver_mg_restrict_d', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ('igx_solver_precond_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ('igx_solver_spmv_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ('igx_solver_solve', C.c_int, [C.c_void_p, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(SolveInfo)]),
    ('igx_solver_declare_symmetric', C.c_int, [C.c_void_p]),
    ('igx_solver_values_changed', C.c_int, [C.c_void_p]),
    ('igx_solver_masked_norm_d', C.c_int, [C.c_void_p, C.c_void_p, _dp]),
    ('igx_solver_newton_update_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.POINTER(SolveInfo)]),
    ('igx_solver_create_parabolic', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_void_p)]),
    ('igx_solver_take_values', C.c_int, [C.c_void_p, C.c_int]),
    ('igx_solver_set_dirk', C.c_int, [C.c_void_p, C.c_int, _dp, C.c_double]),
    ('igx_solver_dirk_run', C.c_int, [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_int, _dp,
                                      C.POINTER(C.c_int32), C.POINTER(DirkInfo)]),
    ('igx_solver_set_stepper', C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    ('igx_solver_set_step_precond', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_dp), C.POINTER(_dp)]),
    ('igx_solver_step_begin', C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    ('igx_solver_step_attempt', C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(StepInfo)]),
    ('igx_solver_step_accept', C.c_int, [C.c_void_p]),
    ('igx_solver_step_state', C.c_int, [C.c_void_p, C.c_int, _dp]),
    ('igx_solver_error_ratio_d', C.c_int, [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_void_p), C.c_void_p, C.c_double, _dp]),
    ('igx_solver_set_mass_d', C.c_int, [C.c_void_p, C.c_void_p]),
    ('igx_solver_take_mass', C.c_int, [C.c_void_p]),
    ('igx_solver_eig_set_precond', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_dp), C.POINTER(_dp), C.c_int]),
    ('igx_solver_eig_begin', C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int]),
    ('igx_solver_eig_products', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ('igx_solver_eig_gram', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), _dp]),
    ('igx_solver_eig_combine', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, C.c_int]),
    ('igx_solver_eig_residuals', C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    ('igx_solver_eig_precond', C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ('igx_solver_eig_download', C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp]),
    ('igx_solver_eig_info', C.c_int, [C.c_void_p, C.POINTER(EigInfo)]),
    ('igx_solver_eig_end', C.c_int, [C.c_void_p]),
    ('igx_solver_eig_products_d', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('igx_solver_eig_gram_d', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), _dp]),
    ('igx_solver_eig_combine_d', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), _dp, C.c_void_p]),
    ('igx_solver_eig_residuals_d', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, _dp, C.c_void_p, _dp, _dp]),
    ('igx_solver_eig_precond_d', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ('igx_kron_apply_d', C.c_int, [C.c_void_p, C.POINTER(KronDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    ('igx_pair_create', C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_dp)]),
    ('igx_pair_destroy', None, [C.c_void_p]),
    ('igx_pair_get_info', C.c_int, [C.c_void_p, C.POINTER(PairInfo)]),
    ('igx_pair_pattern', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ('igx_pair_assemble', C.c_int, [C.c_void_p, C.c_int, _dp]),
    ('igx_pair_entries', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.c_size_t, _dp]),
    ('igx_pair_d_data', C.c_void_p, [C.c_void_p]),
    ('igx_pair_last_timing', C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    ('igx_solver_create_saddle', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_void_p)]),
    ('igx_solver_take_pair_block', C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ('igx_solver_set_saddle_schur', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_dp), C.POINTER(_dp), C.c_int,
                                              _dp, C.c_double]),
    ('igx_solver_saddle_projection', C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    ('igx_solver_download_pair_block', C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp]),
    ('igx_solver_saddle_product_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, _dp]),
    ('igx_solver_saddle_timing', C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ('igx_solver_set_gmres', C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ('igx_solver_gmres_restarts', C.c_int, [C.c_void_p]),
    ('igx_solver_gmres_orth_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, _dp, _dp]),
    ('igx_solver_gmres_combine_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _dp, C.c_void_p]),
    ('igx_solver_gmres_timing', C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ('igx_patch_eval_vspline_d', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p * 12]),
    ('igx_patch_set_form_sum_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    ('igx_solver_replace_block', C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ('igx_solver_hide_block', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ('igx_solver_saddle_residual_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _dp]),
    ('igx_solver_saddle_correct_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(SolveInfo)]),
    ('igx_csr_rap_d', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    ('igx_csr_rect_spmv_d', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_int32]),
    ('igx_hmg_create', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ('igx_hmg_destroy', None, [C.c_void_p]),
    ('igx_hmg_set_matrix', C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    ('igx_hmg_set_transfer', C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp]),
    ('igx_hmg_galerkin', C.c_int, [C.c_void_p, C.c_int, C.c_int32]),
    ('igx_hmg_set_smoother', C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64]),
    ('igx_hmg_set_inverse', C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int64, _dp]),
    ('igx_hmg_set_options', C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ('igx_hmg_set_free', C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    ('igx_hmg_level_values', C.c_int, [C.c_void_p, C.c_int, _dp]),
    ('igx_hmg_level_info', C.c_int, [C.c_void_p, C.c_int, C.POINTER(HmgLevel)]),
    ('igx_hmg_spmv_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    ('igx_hmg_cycle_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ('igx_hmg_solve_d', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(HmgInfo)]),
    ('igx_hmg_profile_d', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(HmgProfile)]),
]

_lib = None
_lock = threading.Lock()


IGX_OK, IGX_ERR_ARG, IGX_ERR_HIP, IGX_ERR_UNSUPPORTED, IGX_ERR_NOMEM, IGX_ERR_NORTC, IGX_ERR_COMPILE = 0, 1, 2, 3, 4, 5, 6      # include/igx.h
_warned = set()


def sampled_fallback(e, what):
    """May a call that hands an EXPRESSION to the run-time compiler fall back to sampling on the host after error `e`?  Only when
    the device path is not available for this input -- no libhiprtc on the box, the expression does not compile, the kernel does
    not serve the patch -- never after a device failure (IGX_ERR_HIP: failed launch, sticky error) or an allocation failure
    (IGX_ERR_NOMEM): those are re-raised.  The reason is reported once per kind, so that a missing libhiprtc is visible."""
    code = getattr(e, 'code', None)
    if code not in (IGX_ERR_NORTC, IGX_ERR_COMPILE, IGX_ERR_UNSUPPORTED):
        return False
    key = (what, code)
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn('pyiga_amd: %s is sampled on the host (%s)' % (what, str(e).split(': ', 1)[-1][:200]), RuntimeWarning, stacklevel=3)
    return True


class IgxError(RuntimeError):
    """An entry point of libigx returned a status other than IGX_OK; ``code`` carries it (None: raised on the Python side)."""
    code = None


def load():
    """Load libigx.so and declare every prototype.  Raises if the library was not built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise IgxError('%s not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                               '(or `make -C pyiga_amd/csrc`). pyiga_amd has no CPU fallback.' % LIB_PATH)
            lib = C.CDLL(LIB_PATH)
            for name, res, args in SYMBOLS:
                fn = getattr(lib, name)          # AttributeError if the symbol is not exported
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def last_error():
    return load().igx_last_error().decode('utf-8', 'replace')


def check(rc, what):
    if rc != 0:
        e = IgxError('%s failed (code %d): %s' % (what, rc, last_error()))
        e.code = rc
        raise e


def dptr(a):
    return a.ctypes.data_as(_dp)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# -------------------------------------------------------------------------------------------
_ctx = {}


class Context:
    """One per GPU: wraps igx_ctx (device id + HIP stream)."""

    def __init__(self, device=0):
        lib = load()
        self.device = int(device)
        self.handle = lib.igx_create(self.device)
        if not self.handle:
            raise IgxError('igx_create(%d) failed: %s' % (self.device, last_error()))

    def sync(self):
        check(load().igx_sync(self.handle), 'igx_sync')

    def close(self):
        if self.handle:
            load().igx_destroy(self.handle)
            self.handle = None


def default_device():
    """LOCAL_RANK under torch.distributed.run, else IGX_DEVICE, else 0."""
    for key in ('IGX_DEVICE', 'LOCAL_RANK'):
        if key in os.environ:
            return int(os.environ[key])
    return 0


def context(device=None):
    device = default_device() if device is None else int(device)
    with _lock:
        ctx = _ctx.get(device)
    if ctx is None:
        ctx = Context(device)
        with _lock:
            _ctx[device] = ctx
    return ctx


def device_code_sha(path=None):
    """sha256 (first 16 hex digits) of the gfx950 code objects inside the library -- the ``.hip_fatbin`` section of the ELF
    file.  Host-only changes leave it alone: what the committed counter passes (profiles/*traffic.json) were measured on is
    identified by the device code, not by the text of the sources."""
    import hashlib
    import struct
    p = path or LIB_PATH
    with open(p, 'rb') as f:
        eh = f.read(64)
        if eh[:4] != b'\x7fELF' or eh[4] != 2:
            return None
        shoff, = struct.unpack_from('<Q', eh, 0x28)
        shentsize, shnum, shstrndx = struct.unpack_from('<HHH', eh, 0x3A)
        f.seek(shoff)
        sh = [struct.unpack_from('<IIQQQQIIQQ', f.read(shentsize)) for _ in range(shnum)]
        f.seek(sh[shstrndx][4])
        names = f.read(sh[shstrndx][5])
        for name_off, _, _, _, off, size, *_ in sh:
            if names[name_off:names.index(b'\0', name_off)] == b'.hip_fatbin':
                f.seek(off)
                return hashlib.sha256(f.read(size)).hexdigest()[:16]
    return None
