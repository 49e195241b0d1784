"""Hierarchical spline spaces: HB- and THB-splines over an adaptively refined mesh (interface of pyiga/hierarchical.py).

:class:`HSpace` keeps, per level, one boolean array over the cells and one over the functions of the tensor-product mesh for
each of the four sets (active / deactivated cells, active / deactivated functions); every set operation of the refinement rule
is an array operation on them (supports and "supported in" are products of 1D incidence matrices applied axis by axis), as the
``Multipatch`` numbering does it with index arrays.  The public accessors return what the reference returns (sets of
multi-index tuples, tuples of ravelled index arrays).

The **canonical order** of the degrees of freedom: level by level, inside a level by ascending ravelled (C-order) index of the
active functions.

:class:`HDiscretization` assembles a variational form over such a space on the device: one on-demand assembler per level,
restricted to the bounding box of the rows it needs, whose pattern entries stay in device memory, and the level-coupling
contraction ``csrc/hier.hip`` that computes every value of the HB matrix from them.
"""
import ctypes as C

import numpy as np
import scipy.sparse

from . import bspline


################################################################################
# Tensor-product meshes
################################################################################

def _incidence_1d(kv):
    """Cells x functions 0/1 matrix of one axis: entry (c, j) is set when B-spline j does not vanish on cell c."""
    ms = kv.mesh_support_idx_all()
    cnt = ms[:, 1] - ms[:, 0]
    cols = np.repeat(np.arange(ms.shape[0]), cnt)
    rows = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(ms[:, 0], cnt)
    return scipy.sparse.csr_matrix((np.ones(rows.size, dtype=np.int32), (rows, cols)), shape=(kv.numspans, ms.shape[0]))


def _apply_axes(mats, mask):
    """Boolean array: the Kronecker product of the 0/1 matrices `mats` applied to `mask` (one matrix per axis), > 0."""
    X = mask.astype(np.int32)
    for ax, M in enumerate(mats):
        Y = np.moveaxis(X, ax, 0)
        shape = Y.shape
        Y = (M @ Y.reshape(shape[0], -1) > 0).astype(np.int32)
        X = np.moveaxis(Y.reshape((M.shape[0],) + shape[1:]), 0, ax)
    return X > 0


def _mask_of(shape, tuples):
    m = np.zeros(shape, dtype=bool)
    idx = np.asarray(list(tuples), dtype=np.int64).reshape(-1, len(shape))
    if idx.size:
        m[tuple(idx.T)] = True
    return m


def _tuples_of(mask):
    return set(map(tuple, np.argwhere(mask).tolist()))


class TPMesh:
    """One level of the hierarchy: the tensor-product mesh and basis of a tuple of knot vectors.

    The working representation is the pair of 1D incidence matrices per axis (cells x functions and its transpose); the
    boolean-array methods apply them axis by axis.  The tuple-based methods are the public form of the same operations."""

    def __init__(self, kvs):
        kvs = tuple(kvs)
        self._inc = tuple(_incidence_1d(kv) for kv in kvs)
        self._incT = tuple(M.T.tocsr() for M in self._inc)
        self.kvs, self.dim = kvs, len(kvs)
        shapes = [M.shape for M in self._inc]
        self.numspans = [int(sh[0]) for sh in shapes]
        self.numdofs = [int(sh[1]) for sh in shapes]
        self.numel, self.numbf = int(np.prod(self.numspans)), int(np.prod(self.numdofs))
        self.meshsupp = tuple(kv.mesh_support_idx_all() for kv in kvs)

    def __eq__(self, other):
        return isinstance(other, TPMesh) and self.dim == other.dim and all(a == b for a, b in zip(self.kvs, other.kvs))

    def refine(self):
        """The mesh with every span of every axis halved."""
        return TPMesh(tuple(kv.refine() for kv in self.kvs))

    # boolean arrays over the cells / the functions (what HSpace works with)
    def support_mask(self, fmask):
        return _apply_axes(self._inc, fmask)

    def supported_in_mask(self, cmask):
        return _apply_axes(self._incT, cmask)

    # the same with multi-index tuples
    def cells(self):
        """All cells, as a list of multi-indices in C order."""
        return [tuple(c) for c in np.ndindex(*self.numspans)]

    def functions(self):
        """All basis functions, as a list of multi-indices in C order."""
        return [tuple(f) for f in np.ndindex(*self.numdofs)]

    def cell_extents(self, c):
        """Per axis the pair (lower, upper) of the cell with multi-index `c`."""
        meshes = [kv.mesh for kv in self.kvs]
        return tuple((m[j], m[j + 1]) for m, j in zip(meshes, c))

    def support(self, funcs):
        """The cells on which at least one of the functions `funcs` (multi-indices) does not vanish, as a set."""
        return _tuples_of(self.support_mask(_mask_of(self.numdofs, funcs)))

    def supported_in(self, cells):
        """The functions that do not vanish on at least one of the cells `cells` (multi-indices), as a set."""
        return _tuples_of(self.supported_in_mask(_mask_of(self.numspans, cells)))

    def neighbors(self, funcs):
        """The functions whose support overlaps that of one of `funcs`, as a set."""
        return _tuples_of(self.supported_in_mask(self.support_mask(_mask_of(self.numdofs, funcs))))


def _children(cmask):
    """Cells of the next finer level that lie in the given cells."""
    for ax in range(cmask.ndim):
        cmask = np.repeat(cmask, 2, axis=ax)
    return cmask


def _parents(cmask, levels=1):
    """Cells `levels` levels up that contain one of the given cells."""
    for _ in range(levels):
        shape = []
        for n in cmask.shape:
            shape += [n // 2, 2]
        cmask = cmask.reshape(shape).any(axis=tuple(range(1, 2 * cmask.ndim, 2)))
    return cmask


def composite_table(Ps):
    """The 1D two-scale relation over several levels as a table.  `Ps`: the 1D prolongation matrices from the coarse level up,
    possibly none.  Returns ``(C, clo, cnt, w)``: the product ``C = Ps[-1] ... Ps[0]`` (CSC; None without matrices) and, for
    every coarse function ``a``, the first fine child ``clo[a]``, the number of children ``cnt[a]`` and their weights
    ``w[a, :cnt[a]]`` (children of a B-spline under knot insertion are consecutive)."""
    if not Ps:
        return None, None, None, None
    Cm = Ps[0]
    for P in Ps[1:]:
        Cm = P @ Cm
    Cm = scipy.sparse.csc_matrix(Cm)
    Cm.sort_indices()
    cnt = np.diff(Cm.indptr).astype(np.int32)
    clo = Cm.indices[Cm.indptr[:-1]].astype(np.int32)
    pos = np.arange(Cm.nnz) - np.repeat(Cm.indptr[:-1], cnt)
    assert np.array_equal(Cm.indices, np.repeat(clo, cnt) + pos), 'children of a B-spline are not consecutive'
    w = np.zeros((cnt.size, int(cnt.max())))
    w[np.repeat(np.arange(cnt.size), cnt), pos] = Cm.data
    return Cm, clo, cnt, w


def _expand_columns(tables, multi, fine_shape):
    """COO triple of the columns ``kron_ax C_ax[:, multi[ax][n]]``, n = 0 .. N-1, from the per-axis tables (clo, cnt, w) of
    :func:`composite_table`: rows are ravelled fine indices, columns are n."""
    N = multi[0].size
    rows = np.zeros((N, 1), dtype=np.int64)
    vals = np.ones((N, 1))
    ok = np.ones((N, 1), dtype=bool)
    for (clo, cnt, w), a, n_fine in zip(tables, multi, fine_shape):
        m = np.arange(w.shape[1])
        width = rows.shape[1] * m.size
        rows = (rows[:, :, None] * n_fine + (clo[a][:, None] + m[None, :])[:, None, :]).reshape(N, width)
        vals = (vals[:, :, None] * w[a][:, None, :]).reshape(N, width)
        ok = (ok[:, :, None] & (m[None, :] < cnt[a][:, None])[:, None, :]).reshape(N, width)
    cols = np.broadcast_to(np.arange(N)[:, None], rows.shape)
    return rows[ok], cols[ok], vals[ok]


################################################################################
# The hierarchical space
################################################################################

class HSpace:
    """An HB-spline or THB-spline space over an adaptively refined mesh.

    Arguments:
        kvs: the `d` knot vectors of the tensor-product space of the coarsest level
        truncate (bool): THB-splines if True, HB-splines otherwise
        disparity (int): the mesh level disparity :meth:`refine` keeps: an active function of level `lv` interacts with
            functions of the levels ``lv - disparity .. lv`` only.  ``numpy.inf`` (default): no restriction.
        bdspecs: boundary specifications (``(axis, side)`` or names) of the sides whose degrees of freedom
            :meth:`dirichlet_dofs` lists
    """

    def __init__(self, kvs, truncate=False, disparity=np.inf, bdspecs=None):
        mesh = TPMesh(kvs)
        self.dim = mesh.dim
        self.truncate = bool(truncate)
        self.disparity = disparity
        self._meshes = [mesh]
        self._P = []                                            # per level: the 1D prolongation matrices to the next one
        self._cact = [np.ones(mesh.numspans, dtype=bool)]
        self._cdeact = [np.zeros(mesh.numspans, dtype=bool)]
        self._fact = [np.ones(mesh.numdofs, dtype=bool)]
        self._fdeact = [np.zeros(mesh.numdofs, dtype=bool)]
        if bdspecs is not None:
            from .form_assemblers import parse_bdspec
            bdspecs = [parse_bdspec(bd, self.dim) for bd in bdspecs]
        self.bdspecs = bdspecs

    # -- levels
    def _add_level(self):
        old = self._meshes[-1]
        new = old.refine()
        self._meshes.append(new)
        self._P.append(tuple(bspline.prolongation(k0, k1) for k0, k1 in zip(old.kvs, new.kvs)))
        self._cact.append(np.zeros(new.numspans, dtype=bool))
        self._cdeact.append(np.zeros(new.numspans, dtype=bool))
        self._fact.append(np.zeros(new.numdofs, dtype=bool))
        self._fdeact.append(np.zeros(new.numdofs, dtype=bool))

    def _ensure_levels(self, L):
        while self.numlevels < L:
            self._add_level()

    @property
    def numlevels(self):
        """The number of levels."""
        return len(self._meshes)

    @property
    def numactive(self):
        """A tuple with the number of active basis functions per level."""
        return tuple(int(m.sum()) for m in self._fact)

    @property
    def numdofs(self):
        """The total number of active basis functions."""
        return sum(self.numactive)

    def mesh(self, lv):
        """The :class:`TPMesh` of level `lv`."""
        return self._meshes[lv]

    def knotvectors(self, lv):
        """The knot vectors of the tensor-product space of level `lv`."""
        return self._meshes[lv].kvs

    # -- cells and functions
    def active_cells(self, lv=None, flat=False):
        """The set of active cells of level `lv`; without `lv` the list of these sets, or with ``flat=True`` the list of
        ``(lv, cell)`` pairs in canonical order."""
        if lv is not None:
            return _tuples_of(self._cact[lv])
        if flat:
            return [(l, tuple(c)) for l in range(self.numlevels) for c in np.argwhere(self._cact[l]).tolist()]
        return [self.active_cells(l) for l in range(self.numlevels)]

    def deactivated_cells(self, lv=None):
        if lv is not None:
            return _tuples_of(self._cdeact[lv])
        return [self.deactivated_cells(l) for l in range(self.numlevels)]

    @property
    def total_active_cells(self):
        return sum(int(m.sum()) for m in self._cact)

    def active_functions(self, lv=None, flat=False):
        """The set of multi-indices of the active functions of level `lv`; without `lv` the list of these sets, or with
        ``flat=True`` the list of ``(lv, multi-index)`` pairs in canonical order."""
        if lv is not None:
            return _tuples_of(self._fact[lv])
        if flat:
            return [(l, tuple(f)) for l in range(self.numlevels) for f in np.argwhere(self._fact[l]).tolist()]
        return [self.active_functions(l) for l in range(self.numlevels)]

    def deactivated_functions(self, lv=None):
        if lv is not None:
            return _tuples_of(self._fdeact[lv])
        return [self.deactivated_functions(l) for l in range(self.numlevels)]

    def cell_extents(self, lv, c):
        """The extents (a tuple of min/max pairs) of the cell `c` of level `lv`."""
        return self._meshes[lv].cell_extents(c)

    def function_support(self, lv, jj):
        """The support (a tuple of min/max pairs) of the function with multi-index `jj` of level `lv`."""
        kvs = self.knotvectors(lv)
        return tuple((kv.mesh[kv.mesh_support_idx(j)[0]], kv.mesh[kv.mesh_support_idx(j)[1]]) for kv, j in zip(kvs, jj))

    def ravel_indices(self, indices):
        """Per level, the ravelled (C-order) indices of the given function multi-indices: `indices` holds one collection per
        level.  A set comes out ascending (it goes through the level's boolean array); a sequence keeps its order."""
        out = []
        for mesh, given in zip(self._meshes, indices):
            if isinstance(given, (set, frozenset)):
                out.append(np.flatnonzero(_mask_of(mesh.numdofs, given)))
                continue
            mi = np.asarray(list(given), dtype=np.int64).reshape(-1, self.dim)
            strides = np.cumprod([1] + mesh.numdofs[:0:-1])[::-1]
            out.append(mi @ strides)
        return tuple(out)

    def active_indices(self):
        """Per level, the ravelled indices of the active basis functions, ascending."""
        return tuple(np.flatnonzero(m) for m in self._fact)

    def deactivated_indices(self):
        """Per level, the ravelled indices of the deactivated basis functions, ascending."""
        return tuple(np.flatnonzero(m) for m in self._fdeact)

    # -- Dirichlet dofs
    def _boundary_mask(self, lv):
        shape = self.mesh(lv).numdofs
        m = np.zeros(shape, dtype=bool)
        for ax, side in (self.bdspecs or ()):
            sl = [slice(None)] * self.dim
            sl[ax] = 0 if side == 0 else -1
            m[tuple(sl)] = True
        return m

    def dirichlet_dofs(self, lv=None):
        """Canonical indices of the degrees of freedom on the sides named by `bdspecs`; with `lv`, in the numbering of that
        level of the virtual hierarchy (the active functions up to `lv`, then the deactivated ones of `lv`)."""
        if lv is None:
            lv = self.numlevels - 1
        out, off = [], 0
        for l in range(lv + 1):
            bd = self._boundary_mask(l).ravel()
            act = np.flatnonzero(self._fact[l])
            out.append(off + np.flatnonzero(bd[act]))
            off += act.size
            if l == lv:
                deact = np.flatnonzero(self._fdeact[l])
                out.append(off + np.flatnonzero(bd[deact]))
        return np.concatenate(out).astype(int)

    def non_dirichlet_dofs(self):
        """Canonical indices of the degrees of freedom that are not on the sides named by `bdspecs`."""
        keep = np.ones(self.numdofs, dtype=bool)
        d = self.dirichlet_dofs()
        keep[d[d < self.numdofs]] = False
        return np.flatnonzero(keep).tolist()

    # -- refinement
    def _cell_support_extension(self, l, cmask, k):
        m = self._meshes[k]
        return m.support_mask(m.supported_in_mask(_parents(cmask, l - k)))

    def _cell_neighborhood(self, l, cmask, truncate):
        d = self.disparity
        if truncate:
            return self._cact[l - d] & _parents(self._cell_support_extension(l, cmask, l - d + 1))
        return self._cact[l - d] & self._cell_support_extension(l, cmask, l - d)

    def _mark_recursive(self, l, marked, truncate):
        while l - self.disparity >= 0:
            nb = self._cell_neighborhood(l, marked[l], truncate)
            if not nb.any():
                return
            l -= self.disparity
            marked[l] = marked[l] | nb

    def refine(self, marked, truncate=False):
        """Refine the given cells: `marked` maps levels to the marked cells of that level.  With a finite disparity coarser
        neighbourhood cells are marked first, recursively (Bracco, Giannelli, Vazquez 2018).

        Returns the cells actually refined, ``{level: set of cells}``."""
        given = {int(lv): list(cells) for lv, cells in marked.items() if len(cells)}
        if not given:
            raise ValueError('refine: no marked cells')
        # refining level l creates cells on l + 1, whose functions need that level's arrays: two levels past the deepest mark
        self._ensure_levels(max(given) + 2)
        L = self.numlevels
        mk = [_mask_of(self._meshes[lv].numspans, given.get(lv, ())) for lv in range(L)]
        if self.disparity < np.inf:
            for l in range(L):
                self._mark_recursive(l, mk, truncate)
        new_cells = [None] * L
        for lv in range(L - 1):
            self._cact[lv] &= ~mk[lv]
            self._cdeact[lv] |= mk[lv]
            new_cells[lv + 1] = _children(mk[lv])
            self._cact[lv + 1] |= new_cells[lv + 1]
        # an active function is deactivated when no cell of its support on its level is still active
        drop = [m.supported_in_mask(mk[lv]) & self._fact[lv] & ~m.supported_in_mask(self._cact[lv]) if mk[lv].any()
                else np.zeros(m.numdofs, dtype=bool) for lv, m in enumerate(self._meshes)]
        for lv in range(L - 1):
            self._fact[lv] &= ~drop[lv]
            self._fdeact[lv] |= drop[lv]
            m = self._meshes[lv + 1]
            cand = m.supported_in_mask(new_cells[lv + 1]) & ~self._fact[lv + 1]
            known = self._cact[lv + 1] | self._cdeact[lv + 1]
            self._fact[lv + 1] |= cand & ~m.supported_in_mask(~known)
        return {lv: _tuples_of(mk[lv]) for lv in range(L) if mk[lv].any()}

    def refine_region(self, lv, region_function):
        """Refine the active cells of level `lv` whose centre satisfies `region_function` (a function of `dim` scalars, the
        coordinates in reversed axis order, e.g. ``(x, y)``)."""
        self._ensure_levels(lv + 2)
        kvs = self.knotvectors(lv)
        cells = np.argwhere(self._cact[lv])
        centres = [0.5 * (kv.mesh[cells[:, ax]] + kv.mesh[cells[:, ax] + 1]) for ax, kv in enumerate(kvs)]
        pick = [tuple(c) for n, c in enumerate(cells.tolist()) if region_function(*(float(ct[n]) for ct in reversed(centres)))]
        return self.refine({lv: pick})

    def copy(self):
        """An independent copy of this space: its own boolean arrays; the (immutable) level meshes and prolongations are shared."""
        other = HSpace.__new__(HSpace)
        other.dim, other.truncate, other.disparity = self.dim, self.truncate, self.disparity
        other.bdspecs = None if self.bdspecs is None else list(self.bdspecs)
        other._meshes, other._P = list(self._meshes), list(self._P)
        for name in ('_cact', '_cdeact', '_fact', '_fdeact'):
            setattr(other, name, [m.copy() for m in getattr(self, name)])
        return other

    # -- representation
    def tp_prolongation(self, lv, kron=False):
        """The prolongation of the tensor-product spaces from level `lv` to `lv` + 1: a tuple of one sparse matrix per axis, or
        with ``kron=True`` their Kronecker product (which deals with the whole tensor-product spaces)."""
        Ps = self._P[lv]
        if not kron:
            return Ps
        K = Ps[0]
        for P in Ps[1:]:
            K = scipy.sparse.kron(K, P, format='csr')
        return scipy.sparse.csr_matrix(K)

    def composite_tables(self, la, k):
        """Per axis, :func:`composite_table` of the prolongations from level `la` to level `k` > `la`."""
        return [composite_table([self._P[l][ax] for l in range(la, k)]) for ax in range(self.dim)]

    def _virtual_indices(self, lv):
        act = list(self.active_indices()[:lv + 1])
        act[lv] = np.concatenate((act[lv], self.deactivated_indices()[lv]))
        return act

    def represent_fine(self, lv=None, truncate=None, rows=None, restrict=False):
        """The matrix that represents the HB- or THB-spline basis functions (``truncate``; default: the attribute) of the
        levels up to `lv` (default: the finest) by their coefficients in the tensor-product space of level `lv`: one column
        per active function in canonical order, then one per deactivated function of level `lv`.

        `rows`: only these rows are filled (``restrict=False``), or the matrix is restricted to them (``restrict=True``)."""
        if lv is None:
            lv = self.numlevels - 1
        assert 0 <= lv < self.numlevels, 'Invalid level.'
        if truncate is None:
            truncate = self.truncate
        act = self._virtual_indices(lv)
        Nf = self.mesh(lv).numbf
        blocks = []
        if not truncate:
            for k in range(lv + 1):
                n = act[k].size
                if k == lv:
                    B = scipy.sparse.csr_matrix((np.ones(n), (act[k], np.arange(n))), shape=(Nf, n))
                else:
                    tabs = [t[1:] for t in self.composite_tables(k, lv)]
                    multi = np.unravel_index(act[k], self.mesh(k).numdofs)
                    I, J, V = _expand_columns(tabs, multi, self.mesh(lv).numdofs)
                    B = scipy.sparse.csr_matrix((V, (I, J)), shape=(Nf, n))
                blocks.append(B)
        else:
            # the functions of level k, prolonged level by level; after every step the coefficients of the active (on `lv`:
            # and deactivated) functions of the level reached are dropped
            Pacc = scipy.sparse.identity(Nf, format='csr')
            for k in reversed(range(lv + 1)):
                if k < lv:
                    keep = np.ones(self.mesh(k + 1).numbf)
                    keep[act[k + 1]] = 0.0
                    Pacc = scipy.sparse.csr_matrix(Pacc @ (scipy.sparse.diags(keep) @ self.tp_prolongation(k, kron=True)))
                blocks.append(Pacc[:, act[k]])
            blocks.reverse()
        R = scipy.sparse.hstack(blocks, format='csr')
        if rows is not None:
            rows = np.asarray(rows, dtype=np.int64)
            if restrict:
                R = R[rows]
            else:
                sel = np.zeros(Nf)
                sel[rows] = 1.0
                R = scipy.sparse.csr_matrix(scipy.sparse.diags(sel) @ R)
        R.eliminate_zeros()
        return R

    def level_restriction(self, lv):
        """The CSR matrix (``mesh(lv).numbf x numdofs``) that maps canonical **HB** coefficients to the coefficients of the
        tensor-product spline of level `lv` that equals the hierarchical function on the active cells of level `lv` (THB
        coefficients go through :meth:`thb_to_hb` first).

        On an active cell of level `lv` only functions of the levels up to `lv` are non-zero, so this is
        ``represent_fine(lv, truncate=False)`` on the rows of the functions whose support meets an active cell of the level,
        restricted to the columns of the active functions of the levels up to `lv` and padded with zero columns."""
        assert 0 <= lv < self.numlevels, 'Invalid level.'
        m = self.mesh(lv)
        rows = np.flatnonzero(m.supported_in_mask(self._cact[lv]))
        n_lv = int(sum(self.numactive[:lv + 1]))
        R = scipy.sparse.csr_matrix(self.represent_fine(lv, truncate=False, rows=rows)[:, :n_lv])
        return scipy.sparse.csr_matrix((R.data, R.indices, R.indptr), shape=(m.numbf, self.numdofs))

    def truncate_one_level(self, k, num_rows=None, inverse=False):
        """The matrix of the truncation from level `k` to `k` + 1 (``inverse=True``: of its inverse)."""
        nt = np.cumsum(self.numactive)
        if num_rows is None:
            num_rows = int(nt[-1])
        A = scipy.sparse.coo_matrix(self.represent_fine(lv=k + 1, rows=self.active_indices()[k + 1], truncate=False, restrict=True))
        coarse = A.col < nt[k]                                   # the components of the coarser functions in the active ones of k+1
        A = scipy.sparse.csr_matrix((A.data[coarse], (A.row[coarse] + nt[k], A.col[coarse])), shape=(num_rows, num_rows))
        I = scipy.sparse.identity(num_rows, format='csr')
        return I + A if inverse else I - A

    def thb_to_hb(self):
        """The square matrix that maps THB-spline coefficients to the HB-spline coefficients of the same function."""
        T = scipy.sparse.identity(self.numdofs, format='csr')
        for k in range(self.numlevels - 1):
            T = self.truncate_one_level(k) @ T
        return scipy.sparse.csr_matrix(T)

    def hb_to_thb(self):
        """The square matrix that maps HB-spline coefficients to the THB-spline coefficients of the same function."""
        T = scipy.sparse.identity(self.numdofs, format='csr')
        for k in range(self.numlevels - 1):
            T = T @ self.truncate_one_level(k, inverse=True)
        return scipy.sparse.csr_matrix(T)

    def split_coeffs(self, x):
        """The coefficient vector `x` (canonical order) split into one vector per level."""
        x = np.asarray(x)
        assert x.shape[0] == self.numdofs, 'Wrong length of input vector'
        return np.split(x, np.cumsum(self.numactive)[:-1])

    # -- the virtual hierarchy of the local multigrid: smoothing sets and prolongators
    # Level `lv` of the virtual hierarchy is the space of the active functions of the levels up to `lv` and the deactivated ones
    # of `lv`.  The four index-set families list, per virtual level and per level, the functions a smoother visits (sorted
    # multi-index tuples, Dirichlet functions left out), as the reference returns them.
    def _refinement_mask(self, lv):
        return self._fact[lv] | self._fdeact[lv]

    def _level_within_disparity(self, i, lv):
        return lv - self.disparity <= i < lv

    @staticmethod
    def _sorted_tuples(mask):
        return [tuple(t) for t in np.argwhere(mask).tolist()]

    def _family(self, coarse_mask):
        """The index-set family whose entry (lv, lv) is `new_indices` and whose entry (lv, i), i < lv within the disparity, is
        the active non-Dirichlet functions of level i inside ``coarse_mask(lv, i)``."""
        out = self.new_indices()
        for lv in range(self.numlevels):
            for i in range(lv):
                if self._level_within_disparity(i, lv):
                    out[lv][i] = self._sorted_tuples(coarse_mask(lv, i) & self._fact[i] & ~self._boundary_mask(i))
        return out

    def new_indices(self):
        """Per virtual level, per level: the functions the level adds (its active, then its deactivated functions)."""
        out = [[[] for _ in range(self.numlevels)] for _ in range(self.numlevels)]
        for lv in range(self.numlevels):
            inner = ~self._boundary_mask(lv)
            out[lv][lv] = self._sorted_tuples(self._fact[lv] & inner) + self._sorted_tuples(self._fdeact[lv] & inner)
        return out

    def _pattern_1d(self, lv):
        """Per axis the 0/1 pattern (fine x coarse) of the two-scale relation from level `lv` to `lv` + 1."""
        return [scipy.sparse.csr_matrix((scipy.sparse.csr_matrix(P) != 0).astype(np.int32)) for P in self._P[lv]]

    def trunc_indices(self):
        """`new_indices` and, per coarser level within the disparity, the active functions that the truncation at the virtual
        level changes: those whose descendants, followed down level by level with the functions of every refinement region
        taken out on the way, meet the refinement region of the virtual level."""
        out = self.new_indices()
        for i in range(self.numlevels - 1):
            act = np.flatnonzero(self._fact[i])
            if act.size == 0:
                continue
            inner = ~self._boundary_mask(i).ravel()[act]
            # row n: the descendants of active function n on the current level (ravelled), as a sparse 0/1 matrix
            M = scipy.sparse.csr_matrix((np.ones(act.size, dtype=np.int32), (np.arange(act.size), act)), shape=(act.size, self.mesh(i).numbf))
            for lv in range(i + 1, self.numlevels):
                if not self._level_within_disparity(i, lv):
                    break
                pats = self._pattern_1d(lv - 1)
                K = pats[0]
                for Pm in pats[1:]:
                    K = scipy.sparse.kron(K, Pm, format='csr')
                M = scipy.sparse.csr_matrix(M @ K.T)
                region = self._refinement_mask(lv).ravel()
                hit = np.asarray(M @ region.astype(np.int32)).ravel() > 0
                M = scipy.sparse.csr_matrix(M @ scipy.sparse.diags((~region).astype(np.int32)))
                M.eliminate_zeros()
                M.data[:] = 1
                pick = np.zeros(self.mesh(i).numbf, dtype=bool)
                pick[act[hit & inner]] = True
                out[lv][i] = self._sorted_tuples(pick.reshape(self.mesh(i).numdofs))
        return out

    def func_supp_indices(self):
        """`new_indices` and, per coarser level, the active ancestors of the active functions of the virtual level."""
        def ancestors(lv, i):
            m = self._fact[lv]
            for l in range(lv - 1, i - 1, -1):
                m = _apply_axes([Pm.T.tocsr() for Pm in self._pattern_1d(l)], m)
            return m
        return self._family(ancestors)

    def cell_supp_indices(self, remove_dirichlet=True):
        """`new_indices` and, per coarser level, the active functions whose support meets that of the active functions of the
        virtual level (support extension)."""
        def extension(lv, i):
            return self.mesh(i).supported_in_mask(_parents(self.mesh(lv).support_mask(self._fact[lv]), lv - i))
        if remove_dirichlet:
            return self._family(extension)
        out = self.new_indices()
        for lv in range(self.numlevels):
            for i in range(lv):
                if self._level_within_disparity(i, lv):
                    out[lv][i] = self._sorted_tuples(extension(lv, i) & self._fact[i])
        return out

    def global_indices(self, vlvl=None):
        """Per level, all functions of virtual level `vlvl` (its active, then its deactivated functions on the last level);
        without `vlvl` the list over all virtual levels."""
        if vlvl is None:
            return [self.global_indices(vlvl=j) for j in range(self.numlevels)]
        out = [[] for _ in range(self.numlevels)]
        for i in range(vlvl + 1):
            out[i] = self._sorted_tuples(self._fact[i])
        out[vlvl] = out[vlvl] + self._sorted_tuples(self._fdeact[vlvl])
        return out

    def indices_to_smooth(self, strategy='func_supp'):
        """Per virtual level, the matrix indices the smoother of that level visits: strategy ``'new'``, ``'trunc'``,
        ``'func_supp'`` or ``'cell_supp'``."""
        assert strategy in ('new', 'trunc', 'func_supp', 'cell_supp'), 'Invalid smoothing strategy'
        chosen = getattr(self, strategy + '_indices')()
        return [self.raveled_to_virtual_canonical_indices(lv, self.ravel_indices(chosen[lv])) for lv in range(self.numlevels)]

    def raveled_to_virtual_canonical_indices(self, lv, indices):
        """Matrix indices on virtual level `lv` of the functions given per level by ravelled tensor-product indices."""
        avail = self._virtual_indices(lv)
        out, off = [], 0
        for l in range(self.numlevels):
            given = np.asarray(indices[l], dtype=np.int64)
            if l > lv:
                if given.size:
                    raise ValueError('level %d has no functions on virtual level %d' % (l, lv))
                continue
            rank = np.full(self.mesh(l).numbf, -1, dtype=np.int64)
            rank[avail[l]] = np.arange(avail[l].size)
            if given.size and rank[given].min() < 0:
                raise ValueError('a function of level %d does not belong to virtual level %d' % (l, lv))
            out.append(off + rank[given])
            off += avail[l].size
        return np.concatenate(out).astype(int) if out else np.zeros(0, dtype=int)

    def virtual_hierarchy_prolongators(self, truncate=None):
        """The prolongation matrices between consecutive virtual levels (scipy sparse, one per level but the finest): the
        identity on the functions kept, the two-scale relation from the deactivated functions of the level to the refinement
        region of the next one, and for THB-splines (``truncate``; default: the attribute) the inverse truncation of that level
        applied from the left."""
        if truncate is None:
            truncate = self.truncate
        IA, ID = self.active_indices(), self.deactivated_indices()
        nt = np.cumsum([a.size for a in IA])
        out = []
        for lv in range(self.numlevels - 1):
            IR = np.concatenate((IA[lv + 1], ID[lv + 1]))
            rank = np.full(self.mesh(lv + 1).numbf, -1, dtype=np.int64)
            rank[IR] = np.arange(IR.size)
            tabs = [t[1:] for t in self.composite_tables(lv, lv + 1)]
            I, J, V = _expand_columns(tabs, np.unravel_index(ID[lv], self.mesh(lv).numdofs), self.mesh(lv + 1).numdofs)
            keep = rank[I] >= 0
            P_rd = scipy.sparse.csr_matrix((V[keep], (rank[I][keep], J[keep])), shape=(IR.size, ID[lv].size))
            P = scipy.sparse.bmat(((scipy.sparse.identity(int(nt[lv])), None), (None, P_rd)), format='csc')
            if truncate:
                P = scipy.sparse.csc_matrix(self.truncate_one_level(lv, num_rows=P.shape[0], inverse=True) @ P)
            out.append(P)
        return out

    # -- evaluation
    def coeffs_to_levelwise_funcs(self, coeffs, truncate=None):
        """One :class:`.BSplineFunc` per level whose sum is the hierarchical spline with the given coefficients (THB-spline
        coefficients with ``truncate=True``; default: the attribute)."""
        if truncate is None:
            truncate = self.truncate
        coeffs = np.asarray(coeffs, dtype=float)
        if truncate:
            coeffs = self.thb_to_hb() @ coeffs
        funcs = []
        for lv, (u, idx) in enumerate(zip(self.split_coeffs(coeffs), self.active_indices())):
            full = np.zeros(self.mesh(lv).numbf)
            full[idx] = u
            funcs.append(bspline.BSplineFunc(self.knotvectors(lv), full))
        return tuple(funcs)

    def grid_eval(self, coeffs, gridaxes, truncate=None):
        """The hierarchical spline with the given coefficients on a tensor-product grid."""
        return sum(f.grid_eval(gridaxes) for f in self.coeffs_to_levelwise_funcs(coeffs, truncate=truncate))


class HSplineFunc:
    """A scalar function in a hierarchical spline space: `u` are the coefficients of the active basis functions in canonical
    order, THB-spline coefficients with ``truncate=True`` (default: the attribute of the space).  The level-wise tensor-product
    splines are evaluated on the device and summed."""

    dim = 1                                                      # scalar functions only

    def __init__(self, hspace, u, truncate=None):
        u = np.asarray(u, dtype=float)
        if u.shape != (hspace.numdofs,):
            raise ValueError('HSplineFunc: %r coefficients, the space has %d active functions' % (u.shape, hspace.numdofs))
        self.hs, self.coeffs = hspace, u
        self.truncate = bool(hspace.truncate if truncate is None else truncate)

    @property
    def sdim(self):
        return self.hs.dim

    def output_shape(self):
        return ()

    def _funcs(self):
        return self.hs.coeffs_to_levelwise_funcs(self.coeffs, truncate=self.truncate)

    @property
    def support(self):
        return tuple(kv.support() for kv in self.hs.knotvectors(0))

    def grid_eval(self, gridaxes):
        return sum(f.grid_eval(gridaxes) for f in self._funcs())

    def grid_jacobian(self, gridaxes):
        return sum(f.grid_jacobian(gridaxes) for f in self._funcs())

    def grid_hessian(self, gridaxes):
        return sum(f.grid_hessian(gridaxes) for f in self._funcs())

    def eval(self, *x):
        """The value at one point, coordinates in reversed axis order (``f.eval(x, y)``)."""
        assert len(x) == self.sdim, 'Input has wrong dimension'
        grid = [np.array([float(c)]) for c in reversed(x)]
        return float(np.asarray(self.grid_eval(grid)).ravel()[0])

    __call__ = eval


def mark(hs, eta2, theta=0.5, strategy='dorfler'):
    """The cells to refine from the squared indicators `eta2` (one per active cell, in the order of
    ``hs.active_cells(flat=True)``): ``{level: set of cell tuples}``, ready for ``hs.refine``.

    ``'dorfler'``: the cells sorted by `eta2` descending (ties: canonical position ascending), the shortest prefix whose sum is at
    least ``theta * sum(eta2)``, summed in that order.  ``'max'``: the cells with ``eta2 >= theta^2 max(eta2)``."""
    eta2 = np.asarray(eta2, dtype=np.float64).ravel()
    cells = hs.active_cells(flat=True)
    if eta2.size != len(cells):
        raise ValueError('mark: %d indicators for %d active cells' % (eta2.size, len(cells)))
    if not (0.0 < theta <= 1.0):
        raise ValueError('mark: theta = %r, expected 0 < theta <= 1' % (theta,))
    if not np.all(eta2 >= 0.0):
        raise ValueError('mark: squared indicators are not negative (or NaN)')
    if strategy == 'dorfler':
        order = np.argsort(-eta2, kind='stable')
        csum = np.cumsum(eta2[order])
        # (all indicators zero: the empty prefix already reaches theta * 0)
        n = int(np.searchsorted(csum, theta * csum[-1], side='left')) + 1 if eta2.size and csum[-1] > 0.0 else 0
        picked = order[:min(n, eta2.size)]
    elif strategy == 'max':
        picked = np.flatnonzero(eta2 >= theta * theta * eta2.max()) if eta2.size else np.zeros(0, dtype=np.int64)
    else:
        raise ValueError("mark: unknown strategy %r ('dorfler' or 'max')" % (strategy,))
    out = {}
    for i in picked.tolist():
        lv, c = cells[i]
        out.setdefault(lv, set()).add(c)
    return out


################################################################################
# Discretisation: host planning of the level-coupling contraction
################################################################################

def _overlap_ranges(kv):
    """Per function of one axis, the first overlapping function and the number of overlapping functions (same space)."""
    s = kv.mesh_support_idx_all()
    first = np.searchsorted(s[:, 1], s[:, 0], side='right')
    last = np.searchsorted(s[:, 0], s[:, 1], side='left')
    return first.astype(np.int32), (last - first).astype(np.int32)


def _coarse_ranges(kv_c, kv_f, gap):
    """Per fine function of one axis, the range [lo, hi) of the functions of the level `gap` levels up whose support overlaps
    its own."""
    sf = kv_f.mesh_support_idx_all()
    sc = kv_c.mesh_support_idx_all()
    clo = sf[:, 0] >> gap
    chi = ((sf[:, 1] - 1) >> gap) + 1                             # coarse cells [clo, chi)
    lo = np.searchsorted(sc[:, 1], clo, side='right')            # first coarse function with hi > clo
    hi = np.searchsorted(sc[:, 0], chi, side='left')             # first coarse function with lo >= chi
    return lo, hi


def _box_pairs(lo, hi, shape_a):
    """All (n, ravelled a) with lo[ax][n] <= a_ax < hi[ax][n]; `n` numbers the rows of the range arrays."""
    N = lo[0].size
    a = np.zeros((N, 1), dtype=np.int64)
    ok = np.ones((N, 1), dtype=bool)
    for l, h, n_a in zip(lo, hi, shape_a):
        m = np.arange(int((h - l).max()) if N else 0)
        width = a.shape[1] * m.size
        a = (a[:, :, None] * n_a + (l[:, None] + m[None, :])[:, None, :]).reshape(N, width)
        ok = (ok[:, :, None] & (m[None, :] < (h - l)[:, None])[:, None, :]).reshape(N, width)
    n = np.broadcast_to(np.arange(N)[:, None], a.shape)
    return n[ok], a[ok]


def plan(hs):
    """Host plan of the contraction for the HB basis of `hs`: the CSR pattern (support overlap of the active functions,
    restricted to level gaps within a finite disparity), and per level the needed rows and the work items.  Vectorised numpy;
    no loop over entries.

    Returns a dict with ``indptr``, ``indices`` (int32), ``levels``: a list (one per level k) of dicts with ``rows`` (needed
    ravelled rows, ascending), ``bbox_rows`` and ``blocks``: a list of dicts per coarser-or-equal level ``la`` with ``la``,
    ``ia``, ``ib`` (ravelled indices on their levels), ``pos`` (position of A[a, b]) and ``pos2`` (position of A[b, a]; -1 on
    the diagonal)."""
    L = hs.numlevels
    act = hs.active_indices()
    na = np.array([a.size for a in act], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(na)))
    N = int(off[-1])
    rank = []
    for lv in range(L):
        r = np.full(hs.mesh(lv).numbf, -1, dtype=np.int64)
        r[act[lv]] = off[lv] + np.arange(na[lv])
        rank.append(r)
    levels = []
    rows_all, cols_all = [], []
    for k in range(L):
        mk = hs.mesh(k)
        shape_k = tuple(mk.numdofs)
        bmulti = np.unravel_index(act[k], shape_k)
        blocks = []
        child_mask = np.zeros(shape_k, dtype=bool)
        la_min = 0 if not np.isfinite(hs.disparity) else max(0, k - int(hs.disparity))
        for la in range(la_min, k + 1):
            if na[k] == 0 or na[la] == 0:
                continue
            ma = hs.mesh(la)
            shape_a = tuple(ma.numdofs)
            if la == k:
                fl = [_overlap_ranges(kv) for kv in mk.kvs]
                lo = [f[bm] for (f, c), bm in zip(fl, bmulti)]
                hi = [(f + c)[bm] for (f, c), bm in zip(fl, bmulti)]
            else:
                rg = [_coarse_ranges(kc, kf, k - la) for kc, kf in zip(ma.kvs, mk.kvs)]
                lo = [r[0][bm] for r, bm in zip(rg, bmulti)]
                hi = [r[1][bm] for r, bm in zip(rg, bmulti)]
            n, ia = _box_pairs(lo, hi, shape_a)
            ib = act[k][n]
            keep = rank[la][ia] >= 0
            if la == k:
                keep &= ia <= ib
            ia, ib = ia[keep], ib[keep]
            if ia.size == 0:
                continue
            blocks.append({'la': la, 'ia': ia, 'ib': ib})
            rows_all += [rank[la][ia], rank[k][ib][ia != ib] if la == k else rank[k][ib]]
            cols_all += [rank[k][ib], rank[la][ia][ia != ib] if la == k else rank[la][ia]]
            if la < k:
                # the children on level k of the coarse functions that interact
                amask = np.zeros(shape_a, dtype=bool)
                amask.ravel()[np.unique(ia)] = True
                tabs = hs.composite_tables(la, k)
                child_mask |= _apply_axes([(t[0] != 0).astype(np.int32).tocsr() for t in tabs], amask)
        needed = hs._fact[k].copy()
        if child_mask.any():
            needed |= child_mask & mk.supported_in_mask(mk.support_mask(hs._fact[k]))
        levels.append({'rows': np.flatnonzero(needed), 'blocks': blocks})
    if rows_all:
        keys = np.concatenate(rows_all) * N + np.concatenate(cols_all)
    else:
        keys = np.zeros(0, dtype=np.int64)
    skeys = np.sort(keys)
    assert skeys.size < 2 ** 31, 'pattern too large for int32 positions'
    assert skeys.size < 2 or (np.diff(skeys) > 0).all(), 'an entry of the pattern was produced twice'
    indices = (skeys % max(N, 1)).astype(np.int32)
    indptr = np.concatenate(([0], np.cumsum(np.bincount(skeys // max(N, 1), minlength=N)))).astype(np.int32)
    for k, lev in enumerate(levels):
        for blk in lev['blocks']:
            ra, rb = rank[blk['la']][blk['ia']], rank[k][blk['ib']]
            blk['pos'] = np.searchsorted(skeys, ra * N + rb).astype(np.int32)
            pos2 = np.searchsorted(skeys, rb * N + ra).astype(np.int32)
            pos2[ra == rb] = -1
            blk['pos2'] = pos2
    return {'indptr': indptr, 'indices': indices, 'levels': levels, 'n': N}


def level_layout(kvs, rows):
    """Layout of the resident entries of one level: the needed `rows` (ravelled, ascending) get the slots 0, 1, ..; the slot
    map covers their bounding box in dof indices; row slot s holds the entries of its tensor-product stencil (columns
    ``first[ax][i_ax] .. + cnt[ax][i_ax]`` per axis, last axis fastest) from ``rowptr[s]`` on.

    Returns a dict with ``first``, ``cnt`` (per axis), ``box_lo``, ``box_n`` (per axis), ``slot`` (int32, -1 = no slot),
    ``rowptr`` (int64) and ``pairs`` ((M, 2) uintp: the index pairs of all entries in this order)."""
    shape = tuple(kv.numdofs for kv in kvs)
    fc = [_overlap_ranges(kv) for kv in kvs]
    multi = np.unravel_index(rows, shape)
    box_lo = [int(m.min()) for m in multi]
    box_n = [int(m.max()) - lo + 1 for m, lo in zip(multi, box_lo)]
    slot = np.full(int(np.prod(box_n)), -1, dtype=np.int32)
    slot[np.ravel_multi_index([m - lo for m, lo in zip(multi, box_lo)], box_n)] = np.arange(rows.size, dtype=np.int32)
    lo = [f[m] for (f, c), m in zip(fc, multi)]
    hi = [(f + c)[m] for (f, c), m in zip(fc, multi)]
    width = np.ones(rows.size, dtype=np.int64)
    for l, h in zip(lo, hi):
        width *= (h - l)
    rowptr = np.concatenate(([0], np.cumsum(width))).astype(np.int64)
    n, cols = _box_pairs(lo, hi, shape)                          # (row-major in n, then the stencil with the last axis fastest)
    pairs = np.empty((cols.size, 2), dtype=np.uintp)
    pairs[:, 0] = rows[n]
    pairs[:, 1] = cols
    return {'first': [f for f, c in fc], 'cnt': [c for f, c in fc], 'box_lo': box_lo, 'box_n': box_n, 'slot': slot,
            'rowptr': rowptr, 'pairs': pairs}


def identity_table(n):
    """The table of :func:`composite_table` for a level paired with itself."""
    return np.arange(n, dtype=np.int32), np.ones(n, dtype=np.int32), np.ones((n, 1))


_SYMMETRIC_FORMS = ('stiffness', 'mass')


class HDiscretization:
    """The discretisation of a variational problem over a hierarchical spline space, assembled on the device.

    Args:
        hspace (:class:`HSpace`): the HB- or THB-spline space
        problem (str): the bilinear form: ``'inner(grad(u),grad(v))*dx'``, ``'u*v*dx'`` or any scalar first-order form string
            of the on-demand general assemblers
        asm_args (dict): the named inputs of the form; at least ``{'geo': geo}``.  The right-hand side draws ``f`` from it.

    After :meth:`assemble_matrix` the HB values stay on the device: ``values_d`` (device pointer), ``indptr``, ``indices``.
    ``max_blocks`` caps the grid of the contraction kernel (None: the library's default).  ``timing`` holds the wall-clock
    times of the last assembly in seconds; with ``timed=True`` every contraction launch is bracketed by events and waited for,
    and ``timing['contract_s']`` is their sum (otherwise 0: the launches are not waited for one by one)."""

    def __init__(self, hspace, problem, asm_args, max_blocks=None, timed=False):
        from . import assemble, forms
        self.hs = hspace
        self.truncate = hspace.truncate
        self.asm_args = dict(asm_args or {})
        if not isinstance(problem, str):
            raise NotImplementedError('hierarchical spaces: the problem is a form string')
        if hspace.dim not in (2, 3):
            raise NotImplementedError('hierarchical spaces are assembled in 2D and 3D')
        if 'geo' not in self.asm_args:
            raise ValueError("required input parameter 'geo' missing")
        self.problem = problem
        self.kind = assemble._KNOWN_FORMS.get(assemble._normalise_form(problem))
        if self.kind == 'convdiff':
            self.kind = None
        _refuse_inputs(self.asm_args)
        self.arity = 2 if self.kind else forms.arity(problem)
        if self.kind is None and self.arity == 2:
            # traced on the host: second / parametric derivatives and non-bilinear forms are refused here
            # the form evaluated once, at one point, with numbers (as the assemblers sample it on the Gauss grid): what the
            # front-end refuses -- second / parametric derivatives, forms that are not bilinear -- is refused here, and a
            # mistake in the string or its inputs shows here as the error it is
            d = hspace.dim
            forms.coefficient_table(problem, (1,) * d, np.full((1,) * d + (d,), 0.5), {k: v for k, v in self.asm_args.items() if k != 'geo'})
        self.max_blocks = max_blocks
        self.timed = bool(timed)
        self.values_d = None
        self.indptr = self.indices = None
        self.timing = {}
        self._plan = None
        self._ctx = None

    # -- device buffers
    def _alloc(self, nbytes):
        from . import _lib
        ptr = _lib.load().igx_dev_alloc(self._ctx.handle, max(int(nbytes), 8))
        if not ptr:
            raise _lib.IgxError('igx_dev_alloc failed: ' + _lib.last_error())
        return ptr

    def _upload(self, arr):
        from . import _lib
        arr = np.ascontiguousarray(arr)
        ptr = self._alloc(arr.nbytes)
        if arr.nbytes:
            _lib.check(_lib.load().igx_dev_upload(self._ctx.handle, ptr, arr.ctypes.data, arr.nbytes), 'igx_dev_upload')
        return ptr

    def _free(self, ptrs):
        from . import _lib
        if self._ctx is not None and getattr(self._ctx, 'handle', None):
            for p in ptrs:
                if p:
                    _lib.load().igx_dev_free(self._ctx.handle, p)

    def close(self):
        """Free the device values."""
        if self.values_d:
            self._free([self.values_d])
            self.values_d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def plan(self):
        """The host plan of the contraction (:func:`plan`), computed once."""
        if self._plan is None:
            self._plan = plan(self.hs)
        return self._plan

    def _level_assembler(self, k, bbox):
        from . import assemblers
        kvs, geo, d = self.hs.knotvectors(k), self.asm_args['geo'], self.hs.dim
        if self.kind:
            cls = {('mass', 2): assemblers.MassAssembler2D, ('mass', 3): assemblers.MassAssembler3D,
                   ('stiffness', 2): assemblers.StiffnessAssembler2D, ('stiffness', 3): assemblers.StiffnessAssembler3D}[(self.kind, d)]
            return cls(kvs, geo, bbox=bbox), self.kind
        cls = assemblers.GeneralFormAssembler2D if d == 2 else assemblers.GeneralFormAssembler3D
        return cls(kvs, geo, self.problem, inputs=self.asm_args, bbox=bbox), 'form'

    def assemble_hb_values(self, symmetric=False):
        """The values of the HB matrix, computed on the device in the order of the pattern of :meth:`plan` and left there
        (``values_d``); returns them as a host array."""
        import time
        from . import _lib, assemble
        if self.arity != 2:
            raise ValueError('the problem is not a bilinear form')
        lib = _lib.load()
        self._ctx = _lib.context(None)
        t0 = time.perf_counter()
        pl = self.plan()
        hs = self.hs
        layouts = [level_layout(hs.knotvectors(k), lev['rows']) if lev['blocks'] else None for k, lev in enumerate(pl['levels'])]
        t_plan = time.perf_counter() - t0
        sym = bool(symmetric) or self.kind in _SYMMETRIC_FORMS
        nnz = int(pl['indices'].size)
        self.close()
        self.indptr, self.indices = pl['indptr'], pl['indices']
        self.values_d = self._alloc(8 * nnz)
        t_setup = t_entries = t_contract = t_tables = 0.0
        ms = C.c_float(0.0)
        for k, lev in enumerate(pl['levels']):
            if not lev['blocks']:
                continue
            lay = layouts[k]
            kvs = hs.knotvectors(k)
            d = hs.dim
            t1 = time.perf_counter()
            asm, kind = self._level_assembler(k, assemble.bbox_for_rows(kvs, lev['rows']))
            tmp = []
            try:
                patch = asm.patch
                patch.upload_pairs(lay['pairs'])
                _lib.check(lib.igx_sync(self._ctx.handle), 'igx_sync')
                t1b = time.perf_counter()
                t_setup += t1b - t1
                patch.entries_resident(kind)
                _lib.check(lib.igx_sync(self._ctx.handle), 'igx_sync')
                t_entries += time.perf_counter() - t1b
                t1c = time.perf_counter()
                d_slot, d_rowptr = self._upload(lay['slot']), self._upload(lay['rowptr'])
                tmp += [d_slot, d_rowptr]
                d_fc = [(self._upload(lay['first'][ax]), self._upload(lay['cnt'][ax])) for ax in range(d)]
                tmp += [p for fc in d_fc for p in fc]
                for blk in lev['blocks']:
                    la = blk['la']
                    shape_a = tuple(kv.numdofs for kv in hs.knotvectors(la))
                    tabs = [t[1:] for t in hs.composite_tables(la, k)] if la < k else [identity_table(n) for n in shape_a]
                    B = _lib.HierBlock()
                    B.dim, B.symmetric = d, int(sym)
                    maxterms = 1
                    for ax in range(d):
                        clo, ccnt, w = tabs[ax]
                        A = B.ax[ax]
                        ptrs = [self._upload(clo.astype(np.int32)), self._upload(ccnt.astype(np.int32)), self._upload(w.astype(np.float64))]
                        tmp += ptrs
                        A.d_clo, A.d_ccnt, A.d_w = ptrs
                        A.d_first, A.d_cnt = d_fc[ax]
                        A.wmax, A.n_coarse, A.n_fine = w.shape[1], shape_a[ax], kvs[ax].numdofs
                        A.box_lo, A.box_n = lay['box_lo'][ax], lay['box_n'][ax]
                        maxterms *= int(min(w.shape[1], lay['cnt'][ax].max()))
                    B.d_slot, B.d_rowptr, B.d_entries = d_slot, d_rowptr, patch._d_val[0]
                    B.n_entries = int(lay['rowptr'][-1])
                    items = [self._upload(blk[name].astype(np.int32)) for name in ('ia', 'ib', 'pos', 'pos2')]
                    tmp += items
                    B.d_ia, B.d_ib, B.d_pos, B.d_pos2 = items
                    B.n_items = int(blk['ia'].size)
                    B.group = 64 if maxterms > 16 else 16
                    B.max_blocks = int(self.max_blocks or 0)
                    t_tables += time.perf_counter() - t1c
                    _lib.check(lib.igx_hier_contract_d(self._ctx.handle, C.byref(B), self.values_d, nnz, C.byref(ms) if self.timed else None), 'igx_hier_contract_d')
                    t_contract += ms.value * 1e-3
                    t1c = time.perf_counter()
                # the launches read the tables and the level entries: wait for them before either is freed
                _lib.check(lib.igx_sync(self._ctx.handle), 'igx_sync')
            finally:
                lib.igx_sync(self._ctx.handle)                   # (also on an error: nothing in flight may read what goes now)
                self._free(tmp)
                asm.patch.close()
        t2 = time.perf_counter()
        vals = np.empty(nnz)
        if nnz:
            _lib.check(lib.igx_dev_download(self._ctx.handle, vals.ctypes.data, self.values_d, vals.nbytes), 'igx_dev_download')
        self.timing = {'plan_s': t_plan, 'level_setup_s': t_setup, 'tables_upload_s': t_tables, 'entries_s': t_entries, 'contract_s': t_contract, 'download_s': time.perf_counter() - t2,
                       'level_entries': int(sum(int(l['rowptr'][-1]) for l in layouts if l is not None)), 'nnz': nnz}
        return vals

    def assemble_matrix(self, symmetric=False):
        """The matrix of the form in the HB- or THB-spline basis: scipy CSR of size ``numdofs``.  ``symmetric=True`` computes
        one orientation of every pair of entries and writes both (the forms known to be symmetric always do)."""
        import time
        n = self.hs.numdofs
        vals = self.assemble_hb_values(symmetric=symmetric)
        A = scipy.sparse.csr_matrix((vals, self.indices, self.indptr), shape=(n, n))
        if self.truncate:
            t0 = time.perf_counter()
            T = self.hs.thb_to_hb()
            A = scipy.sparse.csr_matrix(T.T @ A @ T)
            A.sort_indices()
            self.timing['thb_host_s'] = time.perf_counter() - t0
        return A

    def assemble_rhs(self, problem=None):
        """The right-hand side: by default the L2 inner products with ``asm_args['f']`` (physical coordinates)."""
        return self.assemble_functional('f * v * dx' if problem is None else problem)

    @staticmethod
    def _level_vector_d(asm):
        """Device pointer of the level's whole vector, computed and left on the device (it belongs to the assembler's patch):
        the traced coefficients of v and grad(v) are evaluated at the Gauss points by a generated kernel and contracted there.
        None when the functional was not traced or there is no run-time compiler."""
        from . import _lib
        exprs = getattr(asm, '_jet_exprs', None)
        if exprs is None or not any(e is not None for e in exprs):
            return None
        where = [r for r, e in enumerate(exprs) if e is not None]
        try:
            ptrs, _ = asm.patch.eval_exprs_inputs([exprs[r] for r in where], [])
        except _lib.IgxError as e:
            if not _lib.sampled_fallback(e, 'the jet of a functional'):
                raise
            return None
        jet = [None] * 4
        for r, ptr in zip(where, ptrs):
            jet[r] = ptr
        return asm.patch.load_vector_jet_resident(jet, to_host=False)

    def assemble_functional(self, problem):
        """The vector of a linear functional (a form string with arity 1) over the hierarchical space, canonical order.  The
        vector of every level comes from the device functional assemblers -- on the whole patch of the level: they have no
        bounding box -- and stays on the device when the functional can be traced; the active entries are gathered into
        canonical order there, and the gathered vector is what comes down."""
        from . import _lib, assemblers, forms
        if not isinstance(problem, str):
            raise NotImplementedError('hierarchical spaces: the functional is a form string')
        _refuse_inputs(self.asm_args)
        if forms.arity(problem) != 1:
            raise ValueError('the problem must be a linear functional (arity 1)')
        hs = self.hs
        lib = _lib.load()
        self._ctx = _lib.context(None)
        act = hs.active_indices()
        n = hs.numdofs
        d_out = self._alloc(8 * n)
        try:
            off = 0
            for k in range(hs.numlevels):
                if act[k].size == 0:
                    continue
                cls = assemblers.GeneralFunctionalAssembler2D if hs.dim == 2 else assemblers.GeneralFunctionalAssembler3D
                asm = cls(hs.knotvectors(k), self.asm_args['geo'], problem, inputs=self.asm_args)
                tmp = []
                try:
                    d_vec, n_vec = self._level_vector_d(asm), hs.mesh(k).numbf
                    if d_vec is None:                                 # (not traceable / no run-time compiler: through the host)
                        vec = np.ascontiguousarray(asm.assemble_vector(), dtype=np.float64).ravel()
                        d_vec = self._upload(vec)
                        tmp.append(d_vec)
                    d_idx = self._upload(act[k].astype(np.int64))
                    tmp.append(d_idx)
                    _lib.check(lib.igx_hier_gather_d(self._ctx.handle, d_vec, n_vec, d_idx, act[k].size, C.c_void_p(d_out + 8 * off)), 'igx_hier_gather_d')
                    _lib.check(lib.igx_sync(self._ctx.handle), 'igx_sync')        # (the gather reads what is freed next)
                finally:
                    self._free(tmp)
                    asm.patch.close()
                off += act[k].size
            rhs = np.empty(n)
            if n:
                _lib.check(lib.igx_dev_download(self._ctx.handle, rhs.ctypes.data, d_out, rhs.nbytes), 'igx_dev_download')
        finally:
            self._free([d_out])
        if self.truncate:
            rhs = hs.thb_to_hb().T @ rhs
        return rhs


def _refuse_inputs(args):
    from . import forms
    for name, val in args.items():
        if name != 'geo' and forms.is_spline_input(val):
            raise NotImplementedError('hierarchical spaces: spline-function input %r is not supported' % name)


def assemble_hspace(problem, hs, args, bfuns=None, boundary=None, symmetric=False, format='csr'):
    """``assemble.assemble`` for an :class:`HSpace`: a matrix for a bilinear form, a vector for a linear one.  What is outside
    the scope is refused before anything is created on the device."""
    if bfuns is not None:
        raise NotImplementedError('hierarchical spaces: bfuns= (vector-valued, custom or two-space basis functions) is not supported')
    if boundary is not None:
        raise NotImplementedError('hierarchical spaces: boundary= forms are not supported')
    disc = HDiscretization(hs, problem, args)
    if disc.arity == 1:
        return disc.assemble_functional(problem)
    try:
        return disc.assemble_matrix(symmetric=symmetric).asformat(format)
    finally:
        disc.close()
