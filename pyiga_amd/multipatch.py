"""Multi-patch domains: several tensor-product patches glued at conforming interfaces (names and behaviour of
``pyiga.assemble.Multipatch``, ``detect_interfaces`` and the Dirichlet helpers, pyiga/assemble.py:346-570, 1103-1389).

The dof numbering is the reference's: the non-shared dofs of patch p get ``M_ofs[p]`` plus their rank in tensor-product
order, shared dof ``sd`` gets ``M_ofs[-1] + sd`` in the order ``join_dofs`` creates them.  The global matrix
``sum_p X_p A_p X_p^T`` is formed on the device (``igx_multipatch_*``, pyiga_amd/csrc/multipatch.hip): its pattern once per
``Multipatch``, then one scatter pass per patch straight from the patch's device values.  The sums can also stay on the
device and be solved there: ``pyiga_amd.solvers.MultipatchSystem``.  Vector-valued forms are summed block after block over the
same pattern (``assemble_vector_system``; solved on the device by ``pyiga_amd.solvers.MultipatchVectorSystem``).
"""
import ctypes as C
import itertools
import time
import weakref

import numpy as np
import scipy.sparse

from . import _lib, bspline


################################################################################
# Boundary dofs and Dirichlet conditions (pyiga/assemble.py:346-570)
################################################################################

def slice_indices(ax, idx, shape, ravel=False, flip=None):
    """Dof indices of the slice ``idx`` across axis `ax` of a tensor-product basis of size `shape`: an ``N x dim`` array of
    multi-indices (last axis fastest), or sequential indices with ``ravel=True``.  `flip`: one bool per axis other than
    `ax`; a flipped axis is traversed backwards."""
    shape = tuple(shape)
    if idx < 0:
        idx += shape[ax]
    ranges = [np.arange(n) for n in shape]
    if flip is not None:
        flip = tuple(flip)
        flip = flip[:ax] + (False,) + flip[ax:]
        for k, f in enumerate(flip):
            if f:
                ranges[k] = ranges[k][::-1]
    ranges[ax] = np.array([idx])
    mi = np.stack([g.ravel() for g in np.meshgrid(*ranges, indexing='ij')], axis=1)
    if ravel:
        return np.ravel_multi_index(mi.T, shape)
    return mi


def boundary_dofs(kvs, bdspec, ravel=False, flip=None):
    """Indices of the dofs on the boundary `bdspec` (a name such as ``'left'`` or a pair ``(axis, side)``) of the
    tensor-product basis `kvs`; output as for :func:`slice_indices`."""
    from .form_assemblers import parse_bdspec
    ax, side = parse_bdspec(bdspec, len(kvs))
    return slice_indices(ax, 0 if side == 0 else -1, tuple(kv.numdofs for kv in kvs), ravel=ravel, flip=flip)


def combine_bcs(bcs):
    """One ``(indices, values)`` pair from a sequence of them: indices sorted and unique; a dof that occurs more than once
    takes the value of its first occurrence."""
    bcs = list(bcs)
    indices = np.concatenate([np.asarray(i) for i, _ in bcs])
    values = np.concatenate([np.asarray(v) for _, v in bcs])
    assert indices.shape == values.shape, 'Inconsistent BC sizes'
    uidx, first = np.unique(indices, return_index=True)
    return uidx, values[first]


def _drop_nans(indices, values):
    keep = ~np.isnan(values)
    return (indices, values) if keep.all() else (indices[keep], values[keep])


def compute_dirichlet_bc(kvs, geo, bdspec, dir_func):
    """``(indices, values)`` of the dofs on boundary `bdspec` for the Dirichlet data `dir_func` (physical coordinates; a scalar
    means a constant), interpolated on the boundary face at its Greville points.  A vector-valued `dir_func` gives one dof per
    component in the blocked layout.  NaN values are dropped."""
    from .approx import interpolate
    from .form_assemblers import parse_bdspec
    kvs = tuple(kvs)
    ax, side = parse_bdspec(bdspec, len(kvs))
    assert len(kvs) == geo.sdim, 'Invalid dimension of geometry'
    bdbasis = kvs[:ax] + kvs[ax + 1:]
    if np.isscalar(dir_func):
        value = dir_func
        dir_func = lambda *x: value                   # noqa: E731
    coeffs = interpolate(bdbasis, dir_func, geo=geo.boundary((ax, side)))
    N = tuple(kv.numdofs for kv in kvs)
    idx = slice_indices(ax, 0 if side == 0 else -1, N, ravel=True)
    extra = coeffs.ndim - len(bdbasis)
    if extra == 0:
        return _drop_nans(idx, coeffs.ravel())
    if extra == 1:
        NN = int(np.prod(N))
        return _drop_nans(*combine_bcs((idx + j * NN, coeffs[..., j].ravel()) for j in range(coeffs.shape[-1])))
    raise ValueError('invalid dimension of Dirichlet coefficients: %s' % (coeffs.shape,))


def compute_dirichlet_bcs(kvs, geo, bdconds):
    """Dirichlet conditions on several boundaries: `bdconds` is a list of ``(bdspec, dir_func)`` pairs, or the single pair
    ``('all', dir_func)`` for every boundary.  Returns ``(indices, values)`` as :func:`combine_bcs`."""
    if len(bdconds) == 2 and isinstance(bdconds[0], str) and bdconds[0] == 'all':
        g = bdconds[1]
        bdconds = [((ax, side), g) for ax in range(len(kvs)) for side in (0, 1)]
    return combine_bcs(compute_dirichlet_bc(kvs, geo, bd, g) for bd, g in bdconds)


################################################################################
# Interface detection (pyiga/assemble.py:1107-1178)
################################################################################

def _bbox(geo):
    bb = np.array(geo.bounding_box(), dtype=float)
    return bb[:, 0], bb[:, 1]


def _geo_match(G1, G2, grid=4):
    """(True, flip) if G2 traversed with `flip` equals G1 on a grid of `grid` points per axis, else (False, None)."""
    if G1.sdim != G2.sdim or G1.dim != G2.dim or not np.allclose(G1.support, G2.support):
        return False, None
    pts = [np.linspace(a, b, grid) for a, b in G1.support]
    X1 = G1.grid_eval(pts)
    for flip in itertools.product(*(G2.sdim * [(False, True)])):
        X2 = G2.grid_eval([np.ascontiguousarray(x[::-1]) if f else x for x, f in zip(pts, flip)])
        if np.allclose(X1, X2):
            return True, flip
    return False, None


def detect_interfaces(patches):
    """Matching interfaces between the patches ``[(kvs, geo), ...]``: ``(connected, interfaces)``, `connected` telling whether
    the patch graph is connected, each interface ``(p1, bdspec1, p2, bdspec2, flip)`` ready for
    :meth:`Multipatch.join_boundaries`.  Pairs p1 < p2 whose bounding boxes touch are compared boundary by boundary."""
    import networkx as nx
    boxes = [_bbox(geo) for _, geo in patches]
    diams = [np.linalg.norm(hi - lo) for lo, hi in boxes]
    graph = nx.Graph()
    graph.add_nodes_from(range(len(patches)))
    interfaces = []
    for p1 in range(len(patches)):
        for p2 in range(p1 + 1, len(patches)):
            (lo1, hi1), (lo2, hi2) = boxes[p1], boxes[p2]
            gap = np.linalg.norm(np.maximum(0.0, np.maximum(lo1 - hi2, lo2 - hi1)))
            if not gap < 1e-10 * max(diams[p1], diams[p2]):
                continue
            G1, G2 = patches[p1][1], patches[p2][1]
            assert G1.sdim == G2.sdim and G1.dim == G2.dim
            bds = list(itertools.product(range(G1.sdim), (0, 1)))
            found = False
            for bd1 in bds:
                B1 = G1.boundary(bd1)
                for bd2 in bds:
                    match, flip = _geo_match(B1, G2.boundary(bd2))
                    if match:
                        interfaces.append((p1, bd1, p2, bd2, flip))
                        found = True
            if found:
                graph.add_edge(p1, p2)
    return nx.is_connected(graph), interfaces


################################################################################
# Multipatch (pyiga/assemble.py:1181-1389)
################################################################################

class Multipatch:
    """Patches ``[(kvs, geo), ...]`` with the dofs they share.  With ``automatch=True`` the interfaces are detected
    (:func:`detect_interfaces`), joined and the structure finalized; otherwise call :meth:`join_boundaries` /
    :meth:`join_dofs` and then :meth:`finalize`.  Conforming interfaces only."""

    def __init__(self, patches, automatch=False):
        self.patches = list(patches)
        self.N = [int(bspline.numdofs(kvs)) for kvs, _ in self.patches]
        self.N_ofs = np.concatenate(([0], np.cumsum(self.N)))
        self.shared_per_patch = [dict() for _ in self.patches]
        self.shared_dofs = []
        self.boundary_joins = []                  # the arguments of every join_boundaries call, in order, and whether
        self.bare_joins = False                   # join_dofs was called directly: such joins cannot be replayed on other knots
        self._handle = None
        self._ctx = None                          # the context the handle lives on
        self._pattern = None
        self._solvers = weakref.WeakSet()         # live device solvers over the sums of the handle (destroyed before it)
        self.last_sources, self.last_paths, self.timings = [], [], {}
        if automatch:
            connected, interfaces = detect_interfaces(self.patches)
            if not connected:
                print('WARNING: patch graph is not connected - interface detection may have failed')
            for intf in interfaces:
                self.join_boundaries(*intf)
            self.finalize()

    @property
    def numpatches(self):
        return len(self.patches)

    @property
    def numdofs(self):
        """Number of global dofs (after :meth:`finalize`)."""
        return int(self.M_ofs[-1]) + len(self.shared_dofs)

    def join_dofs(self, p1, I1, p2, I2):
        """Join the dofs `I1` of patch `p1` with the dofs `I2` of patch `p2`."""
        self.bare_joins = True
        self._join_dofs(p1, I1, p2, I2)

    def _join_dofs(self, p1, I1, p2, I2):
        assert len(I1) == len(I2), 'dof arrays must have the same length'
        assert p1 != p2, 'patches must be different'
        self._drop_device()
        spp = self.shared_per_patch
        for i1, i2 in zip(I1, I2):
            i1, i2 = int(i1), int(i2)
            if i1 in spp[p1]:
                sd = spp[p1][i1]
                p, i = p2, i2
            elif i2 in spp[p2]:
                sd = spp[p2][i2]
                p, i = p1, i1
            else:
                sd = len(self.shared_dofs)
                self.shared_dofs.append(set())
                spp[p1][i1] = sd
                self.shared_dofs[sd].add((p1, i1))
                p, i = p2, i2
            spp[p][i] = sd
            self.shared_dofs[sd].add((p, i))

    def join_boundaries(self, p1, bdspec1, p2, bdspec2, flip=None):
        """Join the dofs on boundary `bdspec1` of patch `p1` with those on `bdspec2` of `p2`; `flip` (one bool per axis of the
        boundary) reverses the traversal of `p2`'s boundary along that axis."""
        dofs1 = boundary_dofs(self.patches[p1][0], bdspec1, ravel=True)
        dofs2 = boundary_dofs(self.patches[p2][0], bdspec2, ravel=True, flip=flip)
        self._join_dofs(p1, dofs1, p2, dofs2)
        self.boundary_joins.append((p1, bdspec1, p2, bdspec2, None if flip is None else tuple(flip)))

    def replay_joins(self, patches):
        """A finalized multipatch of `patches` (one per patch of this one, e.g. the same geometries over coarser knot vectors)
        joined as this one was.  ValueError if this one was joined through bare :meth:`join_dofs` calls."""
        if self.bare_joins:
            raise ValueError('the multipatch was joined through join_dofs: its joins cannot be replayed on other knot vectors')
        patches = list(patches)
        if len(patches) != self.numpatches:
            raise ValueError('%d patches given, the multipatch has %d' % (len(patches), self.numpatches))
        MP = Multipatch(patches)
        for join in self.boundary_joins:
            MP.join_boundaries(*join)
        MP.finalize()
        return MP

    def finalize(self):
        """Set up the numbering after all joins."""
        self._drop_device()
        self.M = [n - len(s) for n, s in zip(self.N, self.shared_per_patch)]
        self.M_ofs = np.concatenate(([0], np.cumsum(self.M)))
        self.injective = all(len(set(self.patch_to_global_idx(p).tolist())) == self.N[p] for p in range(self.numpatches))

    def patch_to_global_idx(self, p):
        """Global index of every local (tensor-product) dof of patch `p`."""
        out = np.arange(self.N[p])
        sh = self.shared_per_patch[p]
        loc = np.fromiter(sh.keys(), dtype=out.dtype, count=len(sh))
        sd = np.fromiter(sh.values(), dtype=out.dtype, count=len(sh))
        own = np.setdiff1d(out, loc, assume_unique=True)
        out[own] = np.arange(self.M_ofs[p], self.M_ofs[p] + own.shape[0])
        out[loc] = self.M_ofs[-1] + sd
        return out

    def patch_to_global(self, p, j_global=False):
        """0/1 CSR matrix mapping the dofs of patch `p` to global dofs (with ``j_global``: the columns of all patches'
        dofs, patch p's at ``N_ofs[p]``)."""
        shape = (self.numdofs, int(self.N_ofs[-1]) if j_global else self.N[p])
        ofs = int(self.N_ofs[p]) if j_global else 0
        I = self.patch_to_global_idx(p)
        J = np.arange(ofs, ofs + self.N[p])
        return scipy.sparse.coo_matrix((np.ones(len(I)), (I, J)), shape=shape).tocsr()

    def global_to_patch(self, p):
        """Transpose of :meth:`patch_to_global` (its left inverse)."""
        return self.patch_to_global(p).T

    def compute_dirichlet_bcs(self, bdconds):
        """Dirichlet conditions ``[(patch, bdspec, dir_func), ...]`` as global ``(indices, values)``.  A vector-valued `dir_func`
        gives blocked global indices: the local dof ``c * N_p + i`` of component c becomes ``c * numdofs + l2g_p[i]``, the
        numbering of :meth:`assemble_vector_system` and ``solvers.MultipatchVectorSystem``."""
        bcs, p2g = [], {}
        for p, bdspec, g in bdconds:
            kvs, geo = self.patches[p]
            idx, vals = compute_dirichlet_bc(kvs, geo, bdspec, g)
            if p not in p2g:
                p2g[p] = self.patch_to_global_idx(p)
            comp, loc = np.divmod(idx, self.N[p])
            bcs.append((comp * self.numdofs + p2g[p][loc], vals))
        return combine_bcs(bcs)

    def error_norms(self, u, exact, grad_exact=None):
        """``(l2, h1)`` of ``u_h - exact`` over the whole domain for the global dof vector `u`; `exact` and `grad_exact` as for
        ``approx.error_norms`` (physical coordinates; `h1` is None without `grad_exact`).  The patches are taken in turn, one
        ``DevicePatch`` at a time; the squares are summed and the root is taken once."""
        from . import approx
        u = np.asarray(u, dtype=np.float64).ravel()
        if u.size != self.numdofs:
            raise ValueError('error_norms: %d dofs, the multipatch has %d' % (u.size, self.numdofs))
        sq = np.zeros(2)
        for p, (kvs, geo) in enumerate(self.patches):
            l2, h1 = approx.error_norms(kvs, geo, self.global_to_patch(p) @ u, exact, grad_exact)
            sq += (l2 ** 2, 0.0 if h1 is None else h1 ** 2)
        want_grad = exact is None or grad_exact is not None
        return float(np.sqrt(sq[0])), (float(np.sqrt(sq[1])) if want_grad else None)

    # -- device side
    def _drop_device(self):
        for solver in list(getattr(self, '_solvers', ())):
            solver._release()
        if self._handle:
            _lib.load().igx_multipatch_destroy(self._handle)
        self._handle, self._ctx, self._pattern = None, None, None

    def close(self):
        """Free the device pattern and sums (rebuilt on the next assembly)."""
        self._drop_device()

    def __del__(self):
        try:
            self._drop_device()
        except Exception:
            pass

    def _device(self):
        """The igx_multipatch handle: global pattern and scatter plans, built on first use and kept."""
        if self._handle:
            return self._handle
        from .assemblers import DevicePatch
        from .form_assemblers import _identity_geo
        lib = _lib.load()
        t0 = time.perf_counter()
        dps, maps = [], []
        try:
            for kvs, _ in self.patches:                 # (the pattern depends on the knot vectors only)
                dps.append(DevicePatch(tuple(kvs), _identity_geo(tuple(kvs))))
            maps = [np.ascontiguousarray(self.patch_to_global_idx(p), dtype=np.int32) for p in range(self.numpatches)]
            handles = (C.c_void_p * self.numpatches)(*[d.handle for d in dps])
            ptrs = (C.POINTER(C.c_int32) * self.numpatches)(*[m.ctypes.data_as(C.POINTER(C.c_int32)) for m in maps])
            h = lib.igx_multipatch_create(dps[0].ctx.handle, self.numpatches, handles, ptrs, self.numdofs)
            if not h:
                raise _lib.IgxError('igx_multipatch_create failed: ' + _lib.last_error())
            self._handle, self._ctx = h, dps[0].ctx
        finally:
            for d in dps:
                d.close()
        self.timings['pattern_ms'] = (time.perf_counter() - t0) * 1e3
        return self._handle

    def info(self):
        """Sizes of the global system and the number of local entries per scatter class."""
        inf = _lib.MultipatchInfo()
        _lib.check(_lib.load().igx_multipatch_get_info(self._device(), C.byref(inf)), 'igx_multipatch_get_info')
        return {'nrows': inf.nrows, 'nnz': inf.nnz, 'injective': bool(inf.injective), 'zero_from': inf.zero_from,
                'entries': dict(zip(('direct', 'store', 'rmw', 'atomic'), list(inf.entries)))}

    def pattern(self):
        """(indptr, indices) of the global CSR pattern, int32, built on the device."""
        if self._pattern is None:
            h = self._device()
            nnz = self.info()['nnz']
            indptr = np.empty(self.numdofs + 1, dtype=np.int32)
            indices = np.empty(nnz, dtype=np.int32)
            _lib.check(_lib.load().igx_multipatch_pattern(h, indptr.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          indices.ctypes.data_as(C.POINTER(C.c_int32))), 'igx_multipatch_pattern')
            self._pattern = (indptr, indices)
        return self._pattern

    def _patch_values(self, p, A):
        """Values of the host matrix `A` of patch `p` in the order of the patch's canonical CSR pattern."""
        from .assemblers import DevicePatch
        from .form_assemblers import _identity_geo
        A = scipy.sparse.csr_matrix(A)
        A.sum_duplicates()
        kvs = tuple(self.patches[p][0])
        dp = DevicePatch(kvs, _identity_geo(kvs))
        try:
            indptr, indices = dp.pattern()
        finally:
            dp.close()
        if A.shape == (self.N[p], self.N[p]) and np.array_equal(A.indptr, indptr) and np.array_equal(A.indices, indices):
            return np.ascontiguousarray(A.data, dtype=np.float64)
        n = np.int64(self.N[p])
        keys = np.repeat(np.arange(self.N[p], dtype=np.int64), np.diff(indptr)) * n + indices
        akeys = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr)) * n + A.indices
        pos = np.minimum(np.searchsorted(keys, akeys), keys.shape[0] - 1)
        if not np.array_equal(keys[pos], akeys):
            raise ValueError('patch %d: the matrix has entries outside the tensor-product pattern' % p)
        vals = np.zeros(indices.shape[0])
        vals[pos] = A.data
        return vals

    def _boundary_terms(self, boundary_terms, rhs, args, kwargs, method=None, who='Multipatch.assemble_system'):
        """``{patch index: boundary_terms.PatchTerms}`` of the ``BoundaryTerm`` list, checked and set up on the host (ValueError
        before any device work); a term with a right-hand side needs the sums to have one (`rhs` not None)."""
        from . import boundary_terms as bt
        terms = bt.check_terms(boundary_terms, [len(kvs) for kvs, _ in self.patches], multipatch=True, method=method, who=who)
        if rhs is None and any(t.rhs is not None for t in terms):
            raise ValueError('%s: a boundary term has a right-hand side, but the sums are formed without a load vector (rhs=None)' % who)
        out = {}
        for p in sorted({t.patch for t in terms}):
            kvs, geo = self.patches[p]
            out[p] = bt.PatchTerms(tuple(kvs), geo, [t for t in terms if t.patch == p], method=method, who=who)
        return out

    def assemble_system(self, problem, rhs, args=None, bfuns=None, symmetric=False, format='csr', layout='blocked',
                        boundary_terms=None, **kwargs):
        """System matrix and right-hand side ``(A, b)`` of the bilinear form `problem` and the linear functional `rhs` over
        all patches (arguments as for :func:`pyiga_amd.assemble.assemble`).  Each patch is assembled in turn and scattered
        into the global sums on the device -- from the patch's device values when the assembler leaves them there -- and
        its device memory is freed before the next one.  The pattern keeps entries whose values sum to 0.  `rhs` None: the
        matrix alone, ``b`` is 0.  `boundary_terms`: ``solvers.BoundaryTerm`` objects with their patch index; their face
        matrices are added to the sums on the device after the scatters, their face loads to the patches' load vectors."""
        if bfuns is not None:
            raise NotImplementedError('vector-valued multipatch problems are not supported')
        terms = self._boundary_terms(boundary_terms, rhs, args, kwargs)
        h = self._sum_system(problem, rhs, args, symmetric, format, layout, kwargs, boundary_terms=terms)
        indptr, indices = self.pattern()
        data = np.empty(indices.shape[0])
        b = np.empty(self.numdofs)
        _lib.check(_lib.load().igx_multipatch_download(h, _lib.dptr(data), _lib.dptr(b)), 'igx_multipatch_download')
        A = scipy.sparse.csr_matrix((data, indices.copy(), indptr.copy()), shape=(self.numdofs, self.numdofs))
        return A.asformat(format), b

    # -- vector-valued forms: nc x nc scalar blocks over the one global pattern
    def _vector_assemblers(self, problem, bfuns, args, who):
        """``(nc, assemblers, args)`` of the vector-valued bilinear form `problem`: the checks of
        ``solvers._vector_components`` (ValueError before any device work), then one ``FormAssembler`` per patch with that
        patch's ``geo``.  The caller closes their patches."""
        from . import solvers
        from .form_assemblers import FormAssembler
        args = {k: v for k, v in dict(args or {}).items() if k != 'geo'}
        kvs0, geo0 = self.patches[0]
        nc = solvers._vector_components(problem, tuple(kvs0), dict(args, geo=geo0), bfuns, who=who)
        asms = []
        try:
            for kvs, geo in self.patches:
                asms.append(FormAssembler(tuple(kvs), geo, problem, bfuns=bfuns, inputs=args))
        except Exception:
            for a in asms:
                a.patch.close()
            raise
        return nc, asms, args

    def _sum_vector_blocks(self, assemblers, nc, on_block):
        """The block loop of a vector-valued form, blocks outermost: for every block (p, q) present on any patch the sums are
        restarted, every patch scatters its scalar block -- a patch whose table for this block is absent scatters zeros, since
        ``igx_multipatch_zero`` clears the interface rows only and the interior rows would keep the previous block's values --
        and ``on_block(p, q, handle)`` takes the sums.  Returns ``present[p][q]``; a block absent on every patch is never
        summed.  Restarting the sums makes every ``MultipatchSystem`` over this multipatch stale."""
        from .form_assemblers import _full_table
        lib = _lib.load()
        h = self._device()
        self.pattern()
        absent = lambda tab: all(e is None for row in tab for e in row)          # noqa: E731
        present = [[False] * nc for _ in range(nc)]
        for p in range(nc):
            for q in range(nc):
                tabs = [asm._table[p][q] for asm in assemblers]
                if all(absent(t) for t in tabs):
                    continue
                _lib.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
                for k, (asm, tab) in enumerate(zip(assemblers, tabs)):
                    if absent(tab):
                        zeros = np.zeros(int(asm.patch.nnz))
                        _lib.check(lib.igx_multipatch_scatter_host(h, k, _lib.dptr(zeros)), 'igx_multipatch_scatter_host')
                        continue
                    asm.patch.set_form(_full_table(tab, len(asm.kvs[0])))
                    asm.patch.assemble('form', to_host=False)
                    _lib.check(lib.igx_multipatch_scatter_patch(h, k, asm.patch.handle), 'igx_multipatch_scatter_patch')
                on_block(p, q, h)
                present[p][q] = True
        return present

    def _vector_rhs(self, rhs, test, nc, args):
        """The blocked global right-hand side of ``nc * numdofs`` entries: `rhs` a linear form string in the test function `test`
        (assembled per patch with ``bfuns=[(test, nc)]``, ``layout='blocked'`` and summed on the host with
        ``patch_to_global_idx`` per component), a vector of that length, or a scalar."""
        from . import assemble as asm_mod
        n = self.numdofs
        if isinstance(rhs, str):
            b = np.zeros(nc * n)
            for p, (kvs, geo) in enumerate(self.patches):
                bp = np.asarray(asm_mod.assemble(rhs, tuple(kvs), args=dict(args, geo=geo), bfuns=[(test, nc)], layout='blocked'))
                bp = bp.reshape(nc, self.N[p])
                l2g = self.patch_to_global_idx(p)
                for c in range(nc):
                    np.add.at(b, c * n + l2g, bp[c])
            return b
        if np.ndim(rhs) == 0:
            return np.full(nc * n, float(rhs))
        b = np.ascontiguousarray(rhs, dtype=np.float64).ravel()
        if b.size != nc * n:
            raise ValueError('right-hand side has %d entries, the space %d x %d' % (b.size, nc, n))
        return b

    def assemble_vector_system(self, problem, rhs, bfuns, args=None, format='csr', **kwargs):
        """``(A, b)`` of the vector-valued bilinear form `problem` (``bfuns=[('u', nc), ('v', nc)]``, nc = 2 or 3) and the
        right-hand side `rhs` (a linear form string in the test function, a vector or a scalar) over all patches, in the blocked
        layout: ``nc * numdofs`` entries, component-major, every component with the scalar numbering of the multipatch.  Block
        (p, q) is ``sum_patch X A^patch_pq X^T``, summed on the device over the one global pattern, block after block; the
        pattern keeps entries whose values sum to 0.  Restarts the device sums (a ``MultipatchSystem`` over them goes stale)."""
        from . import solvers
        args = dict(args or {})
        args.update(kwargs)
        nc, asms, args = self._vector_assemblers(problem, bfuns, args, 'Multipatch.assemble_vector_system')
        n = self.numdofs
        try:
            indptr, indices = self.pattern()
            blocks = [[None] * nc for _ in range(nc)]

            def download(p, q, h):
                data = np.empty(indices.shape[0])
                _lib.check(_lib.load().igx_multipatch_download(h, _lib.dptr(data), None), 'igx_multipatch_download')
                blocks[p][q] = scipy.sparse.csr_matrix((data, indices.copy(), indptr.copy()), shape=(n, n))
            self._sum_vector_blocks(asms, nc, download)
        finally:
            for a in asms:
                a.patch.close()
        blocks = [[B if B is not None else scipy.sparse.csr_matrix((n, n)) for B in row] for row in blocks]
        A = scipy.sparse.bmat(blocks, format='csr')
        b = self._vector_rhs(rhs, solvers._test_function_name(problem, bfuns), nc, args)
        return A.asformat(format), b

    def _sum_system(self, problem, rhs, args, symmetric, format, layout, kwargs, on_assembler=None, boundary_terms=None):
        """Restart the device sums and add every patch's matrix and right-hand side to them (the loop of
        :meth:`assemble_system`); returns the handle, the sums left on the device.  `on_assembler(p, asm)` is called with each
        patch's assembler before it assembles.  `rhs` None: the matrices alone (an eigenproblem has no load vector).
        `boundary_terms` (:meth:`_boundary_terms`): the face loads join ``b_p`` before it is scattered (the scatter overwrites
        singly-owned entries), the face matrices are added to the sums after the patch loop; their face patches are closed."""
        boundary_terms = boundary_terms or {}
        try:
            return self._sum_patches(problem, rhs, args, symmetric, format, layout, kwargs, on_assembler, boundary_terms)
        finally:
            for t in boundary_terms.values():
                t.close()

    def _sum_patches(self, problem, rhs, args, symmetric, format, layout, kwargs, on_assembler, boundary_terms):
        from . import assemble as asm_mod
        from . import boundary_terms as bt
        from .assemblers import _DeviceAssembler, _ParametricFormAssembler
        lib = _lib.load()
        h = self._device()
        self.pattern()
        args = dict(args or {})
        args.update(kwargs)
        _lib.check(lib.igx_multipatch_zero(h), 'igx_multipatch_zero')
        self.last_sources, self.last_paths = [], []
        t_asm, t_sc = [], []
        for p in range(self.numpatches):
            kvs, geo = self.patches[p]
            args['geo'] = geo
            t0 = time.perf_counter()
            asm = asm_mod.instantiate_assembler(problem, kvs, args)
            device = (isinstance(asm, _DeviceAssembler) and not isinstance(asm, _ParametricFormAssembler) and layout == 'blocked'
                      and not (symmetric and not getattr(asm, '_symmetric_form', True)))
            try:
                if on_assembler is not None:
                    on_assembler(p, asm)
                if device:
                    asm.patch.assemble(asm._kind, to_host=False)
                    self.last_paths.append(asm.patch.last_path())
                    t1 = time.perf_counter()
                    _lib.check(lib.igx_multipatch_scatter_patch(h, p, asm.patch.handle), 'igx_multipatch_scatter_patch')
                else:
                    vals = self._patch_values(p, asm_mod.assemble_entries(asm, symmetric=symmetric, format='csr', layout=layout))
                    self.last_paths.append(set())
                    t1 = time.perf_counter()
                    _lib.check(lib.igx_multipatch_scatter_host(h, p, _lib.dptr(vals)), 'igx_multipatch_scatter_host')
            finally:
                patch = getattr(asm, 'patch', None)
                if asm is not problem and hasattr(patch, 'close'):      # (device memory of an assembler made here: freed now)
                    patch.close()
            t2 = time.perf_counter()
            self.last_sources.append('device' if device else 'host')
            t_asm.append((t1 - t0) * 1e3)
            t_sc.append((t2 - t1) * 1e3)
            if rhs is None:                           # (no load vector wanted: the summed vector stays 0)
                continue
            b_p = _lib.f64(np.asarray(asm_mod.assemble(rhs, kvs, args=args, symmetric=symmetric, format=format, layout=layout)).ravel())
            if b_p.shape[0] != self.N[p]:
                raise ValueError('patch %d: right-hand side has %d entries, expected %d' % (p, b_p.shape[0], self.N[p]))
            if p in boundary_terms and boundary_terms[p].has_rhs:
                b_p = boundary_terms[p].add_loads(b_p.copy())
            _lib.check(lib.igx_multipatch_scatter_vector(h, p, _lib.dptr(b_p)), 'igx_multipatch_scatter_vector')
        bt.add_to_multipatch(self, h, boundary_terms)
        self.timings.update(assemble_ms=t_asm, scatter_ms=t_sc)
        return h
