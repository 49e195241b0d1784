"""Robin, impedance and Neumann boundary terms of the device-resident systems.

The reference adds them on the host::

    R = assemble('alpha*u*v*ds', kvs, geo=geo, boundary=bd, alpha=alpha)
    bd_dofs = boundary_dofs(kvs, bd, ravel=True)
    A[bd_dofs[:, None], bd_dofs] += R;  b[bd_dofs] += assemble('g*v*ds', kvs, geo=geo, boundary=bd, g=g).ravel()

Here ``BoundaryTerm(bd, matrix='alpha*u*v*ds', rhs='g*v*ds', alpha=alpha, g=g)`` describes one such term and the systems of
``pyiga_amd.solvers`` take a list of them (``boundary_terms=``).  The face matrix is built by ``FormAssembler(..., boundary=bd)``
and added on the device to the volume values the patch (or the multipatch) holds there: for a 3D patch the 2D face patch keeps
its values on the device and ``igx_patch_add_face`` reads them there; the 1D face matrices of 2D patches are formed on the host,
like every 1D matrix of this package, and go up through ``igx_patch_add_face_host``.  The volume matrix never comes down.
"""
import re

import numpy as np

from . import _lib


class BoundaryTerm:
    """One boundary term: on the side `bdspec` (as for ``assemble.assemble(..., boundary=bdspec)``) the scalar bilinear form
    `matrix` (a string in ``u``, ``v`` with ``ds``) is added to the system matrix and the scalar linear form `rhs` (a string in
    ``v`` with ``ds``) to the load vector; either may be None.  `inputs`: the named inputs of the two strings (``geo`` comes from
    the system).  `patch`: the patch index, required by and only valid for a multipatch system."""

    def __init__(self, bdspec, matrix=None, rhs=None, patch=None, **inputs):
        if matrix is None and rhs is None:
            raise ValueError('BoundaryTerm: neither a matrix form nor a right-hand side form given')
        if 'bfuns' in inputs:
            raise ValueError('BoundaryTerm: boundary terms are scalar forms in u and v (no bfuns / vector-valued functions)')
        for what, form, want in (('matrix', matrix, 2), ('rhs', rhs, 1)):
            if form is None:
                continue
            if not isinstance(form, str):
                raise ValueError('BoundaryTerm: %s must be a form string, not %r' % (what, type(form).__name__))
            if re.search(r'\bdx\b', form):
                raise ValueError('BoundaryTerm: %s is a volume integral (dx); a boundary term is written with ds: %r' % (what, form))
            if not re.search(r'\bds\b', form):
                raise ValueError('BoundaryTerm: %s must be a boundary integral (... * ds): %r' % (what, form))
            used = set(re.findall(r'[^\d\W]\w*', form)) & {'u', 'v'}
            if used != ({'u', 'v'} if want == 2 else {'v'}):
                raise ValueError('BoundaryTerm: %s must be %s: %r' % (what, 'bilinear in u and v' if want == 2 else 'linear in v (no u)', form))
        self.bdspec = bdspec
        self.matrix = matrix
        self.rhs = rhs
        self.patch = None if patch is None else int(patch)
        self.inputs = dict(inputs)

    def __repr__(self):
        return 'BoundaryTerm(%r, matrix=%r, rhs=%r, patch=%r)' % (self.bdspec, self.matrix, self.rhs, self.patch)


def _probe(t, d, method, who):
    """The two form strings of term `t` evaluated at ONE point on the host (the centre of the unit cube, a fixed unit normal), as
    ``solvers._check_device_form`` classifies volume forms: ValueError for a form that is not an integral in ds, is vector-valued,
    or -- ``method='cg'`` -- has a physical coefficient table that is not symmetric there.  No geometry and no device: a term
    whose inputs cannot be evaluated at that point is left to the assembler (``PatchTerms`` repeats the symmetry check on the
    face's Gauss grid)."""
    from . import tforms
    from .solvers import symmetric_block_tables
    G = (1,) * (d - 1)
    X = np.full(G + (d,), 0.5)
    normal = np.full(G + (d,), 1.0 / np.sqrt(d))
    inputs = {k: v for k, v in t.inputs.items() if k != 'geo'}
    for what, form, want in (('matrix', t.matrix, 2), ('rhs', t.rhs, 1)):
        if form is None:
            continue
        try:
            arity, measure, table, ncs = tforms.evaluate(form, G, X, inputs, None, normal=normal)
        except Exception:
            continue
        if measure != 'ds' or arity != want or any(nc != 1 for nc in ncs):
            raise ValueError('%s: %r: %s must be a scalar %s boundary integral (... * ds)' % (who, t, what, 'bilinear' if want == 2 else 'linear'))
        if want == 2 and method == 'cg' and not symmetric_block_tables([[table[0][0]]]):
            raise ValueError("%s: %r: method='cg' needs a symmetric boundary matrix, and the coefficient table of this form is not "
                             "symmetric: method='bicgstab'" % (who, t))


def check_terms(terms, dims, multipatch=False, method=None, who='boundary_terms'):
    """The list of `terms` (None: empty) after the checks that need neither geometry nor device -- ValueError for anything that
    is not a ``BoundaryTerm``, an unknown `bdspec`, ``patch=`` given to a one-patch system or missing (or out of range) for a
    multipatch, and what ``_probe`` finds in the form strings.  `dims`: the dimension of the patch, or one per patch of the
    multipatch."""
    from .form_assemblers import parse_bdspec
    terms = list(terms or ())
    for t in terms:
        if not isinstance(t, BoundaryTerm):
            raise ValueError('boundary_terms takes BoundaryTerm objects, not %r' % (type(t).__name__,))
        if multipatch:
            if t.patch is None:
                raise ValueError('%r: a multipatch system needs the patch index of every boundary term (patch=)' % (t,))
            if not 0 <= t.patch < len(dims):
                raise ValueError('%r: patch %d out of range (the multipatch has %d patches)' % (t, t.patch, len(dims)))
            d = dims[t.patch]
        else:
            if t.patch is not None:
                raise ValueError('%r: patch= is for multipatch systems only' % (t,))
            d = dims
        parse_bdspec(t.bdspec, d)
        _probe(t, d, method, who)
    return terms


def face_pattern(tkvs):
    """``(I, J)`` of the canonical CSR pattern of the face space `tkvs` (rows ascending, columns ascending within a row)."""
    from .assemble import _ml_nonzero
    I, J = _ml_nonzero(tkvs, tkvs, False)
    order = np.lexsort((J, I))
    return I[order], J[order]


def face_values(R, tkvs):
    """The values of the face matrix `R` (anything ``scipy.sparse.csr_matrix`` takes; face dofs x face dofs) in the canonical CSR
    order of the face space `tkvs`: what ``igx_patch_add_face_host`` takes.  Entries outside the pattern raise ValueError."""
    import scipy.sparse
    R = scipy.sparse.csr_matrix(R)
    I, J = face_pattern(tkvs)
    vals = np.asarray(R[I, J], dtype=np.float64).ravel()
    P = scipy.sparse.csr_matrix((np.ones(I.shape[0]), (I, J)), shape=R.shape)
    if (abs(R) - abs(R).multiply(P)).count_nonzero():
        raise ValueError('the face matrix has entries outside the tensor-product pattern of the face space')
    return np.ascontiguousarray(vals)


def _symmetric_table(tab, rtol=1e-13):
    """``C[a][b] == C[b][a]`` on the face's Gauss grid, within `rtol` of the largest entry (the rule of
    ``solvers.symmetric_block_tables``)."""
    from .solvers import symmetric_block_tables
    return symmetric_block_tables([[tab]], rtol=rtol)


class PatchTerms:
    """The boundary terms of ONE patch, set up on the host (form strings evaluated on the faces' Gauss grids; no device work),
    then added to device values (``add_matrices``) and to a host load vector (``add_loads``), in the order they were given."""

    def __init__(self, kvs, geo, terms, method=None, who='boundary_terms'):
        from .form_assemblers import FormAssembler
        self.kvs = tuple(kvs)
        self.geo = geo
        self.items = []                              # (term, axis, side, matrix assembler | None, rhs assembler | None)
        d = len(self.kvs)
        for t in terms:
            mat = vec = None
            inputs = {k: v for k, v in t.inputs.items() if k != 'geo'}
            if t.matrix is not None:
                mat = FormAssembler(self.kvs, geo, t.matrix, inputs=inputs, boundary=t.bdspec, lazy_patch=True)
                if mat.arity != 2 or mat._vector_valued:
                    raise ValueError('%s: %r: the matrix must be a scalar bilinear form' % (who, t))
                if method == 'cg' and not _symmetric_table(mat._table[0][0]):
                    raise ValueError("%s: %r: method='cg' needs a symmetric boundary matrix, and the coefficient table of this form "
                                     "is not symmetric on the face's Gauss grid: method='bicgstab'" % (who, t))
            if t.rhs is not None:
                vec = FormAssembler(self.kvs, geo, t.rhs, inputs=inputs, boundary=t.bdspec, lazy_patch=True)
                if vec.arity != 1 or vec._vector_valued:
                    raise ValueError('%s: %r: the right-hand side must be a scalar linear form' % (who, t))
            ax, side = (mat or vec).boundary
            self.items.append((t, ax, side, mat, vec))
        self.has_matrix = any(m is not None for _, _, _, m, _ in self.items)
        self.has_rhs = any(v is not None for _, _, _, _, v in self.items)
        self._d = d

    def symmetric(self):
        """True if every boundary matrix has a symmetric coefficient table (the check ``method='cg'`` makes)."""
        return all(mat is None or _symmetric_table(mat._table[0][0]) for _, _, _, mat, _ in self.items)

    def sigma(self):
        """``1^T R_total 1``: the sum of all entries of all face matrices.  The B-splines of an axis sum to 1 and their
        derivatives to 0, so this is the integral of the value-value coefficient of every table over its face -- a quadrature on
        the host grid the tables already live on; nothing is assembled or reduced for it."""
        from .quadrature import make_tensor_quadrature
        total = 0.0
        for _, _, _, mat, _ in self.items:
            if mat is None or mat._table[0][0][0][0] is None:
                continue
            _, weights = make_tensor_quadrature([kv.mesh for kv in mat._tkvs], mat.nqp)
            W = weights[0] if len(weights) == 1 else weights[0][:, None] * weights[1][None, :]
            total += float(np.sum(W * mat._table[0][0][0][0]))
        return total

    def add_matrices(self, add_face):
        """``add_face(axis, side, face)`` for every matrix term in order; `face` is the face's ``DevicePatch`` holding the values
        on the device (3D volumes) or the host values in the canonical order of the face space (2D volumes)."""
        from .form_assemblers import _assemble_1d_jets, _full_table
        for _, ax, side, mat, _ in self.items:
            if mat is None:
                continue
            tab = mat._table[0][0]
            if all(e is None for row in tab for e in row):
                continue
            if self._d == 3:
                fp = mat.ensure_patch()
                fp.set_form(_full_table(tab, 2))
                fp.assemble('form', to_host=False)             # the face values stay on the device
                add_face(ax, side, fp)
            else:
                A = _assemble_1d_jets(mat._tkvs[0], mat.nqp, C=tab)
                add_face(ax, side, face_values(A, mat._tkvs))

    def add_loads(self, b):
        """``b[bd_dofs] += r`` for every term with a right-hand side, in order; `b`: the patch's load vector (changed in place)."""
        from .multipatch import boundary_dofs
        b = b.reshape(-1)
        for t, ax, side, _, vec in self.items:
            if vec is None:
                continue
            vec.ensure_patch()
            r = np.asarray(vec.assemble_vector(), dtype=np.float64).ravel()
            b[boundary_dofs(self.kvs, (ax, side), ravel=True)] += r
        return b

    def close(self):
        for _, _, _, mat, vec in self.items:
            for a in (mat, vec):
                if a is not None and a.patch is not None:
                    a.patch.close()
                    a.patch = None


def kron_shift(kvs, sigma):
    """The shift ``sigma / (d |parametric domain|)`` per axis that makes the fast-diagonalization preconditioner of a stiffness-like
    form nonsingular when no dof is fixed: ``sigma / |domain|`` is the Rayleigh quotient of the boundary matrices on the constant
    (with respect to the parametric mass matrix), spread over the `d` axes of ``IGX_KRON_SUM``."""
    vol = float(np.prod([kv.support()[1] - kv.support()[0] for kv in kvs]))
    return sigma / vol / len(kvs)


def add_to_multipatch(MP, handle, per_patch):
    """The matrix terms of `per_patch` (patch index -> ``PatchTerms``) added to the sums of the multipatch handle, after all
    scatters, patch after patch and term after term."""
    import ctypes as C
    lib = _lib.load()
    for p in sorted(per_patch):
        def add(ax, side, face, p=p):
            if hasattr(face, 'handle'):
                _lib.check(lib.igx_multipatch_add_face(handle, p, ax, side, face.handle), 'igx_multipatch_add_face')
            else:
                vals = _lib.f64(face).ravel()
                _lib.check(lib.igx_multipatch_add_face_host(handle, p, ax, side, _lib.dptr(vals), C.c_int64(vals.size)),
                           'igx_multipatch_add_face_host')
        per_patch[p].add_matrices(add)
