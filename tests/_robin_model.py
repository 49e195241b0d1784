"""numpy restatement of the position arithmetic of k_face_add (pyiga_amd/csrc/face_add.hip): where the
entries of a face matrix, in the canonical CSR order of the face space, sit among the canonical CSR values of the volume patch.
Only the per-axis tables jlo / jhi / rp enter -- no index arrays, no search -- exactly as on the device."""
import numpy as np


def axis_tables(kv):
    """(jlo, jhi, rp) of one axis: the column range of every row of the 1D pattern and the exclusive prefix sum of its length."""
    from pyiga_amd.assemble import _compute_sparsity_ij
    ij = _compute_sparsity_ij(kv, kv).astype(np.int64)
    N = kv.numdofs
    jlo = np.full(N, np.iinfo(np.int64).max)
    jhi = np.zeros(N, dtype=np.int64)
    np.minimum.at(jlo, ij[:, 0], ij[:, 1])
    np.maximum.at(jhi, ij[:, 0], ij[:, 1] + 1)
    rp = np.concatenate([[0], np.cumsum(jhi - jlo)])
    assert rp[-1] == ij.shape[0]
    return jlo, jhi, rp


def face_kvs(kvs, axis):
    return tuple(kv for k, kv in enumerate(kvs) if k != axis)


def face_nnz(kvs, axis):
    return int(np.prod([axis_tables(kv)[2][-1] for kv in face_kvs(kvs, axis)]))


def face_positions(kvs, axis, side):
    """For every entry of the face matrix of side (axis, side), in the canonical CSR order of the face space, its offset among the
    canonical CSR values of the volume patch.  A 2D patch is a 3D one with a one-dof outer axis, as in the kernel."""
    d = len(kvs)
    tabs = [(np.array([0]), np.array([1]), np.array([0, 1]))] * (3 - d) + [axis_tables(kv) for kv in kvs]
    normal = axis + 3 - d
    (jlo_n, jhi_n, rp_n) = tabs[normal]
    fn = len(jlo_n) - 1 if side else 0
    jn, cn, rpn = fn - jlo_n[fn], jhi_n[fn] - jlo_n[fn], rp_n[fn]
    tu, tv = [k for k in range(3) if k != normal]
    (jlo_u, jhi_u, rp_u), (jlo_v, jhi_v, rp_v) = tabs[tu], tabs[tv]
    S1, S2 = tabs[1][2][-1], tabs[2][2][-1]
    Sv = rp_v[-1]
    out = np.empty(rp_u[-1] * Sv, dtype=np.int64)
    for u in range(len(jlo_u)):
        cu, ru = jhi_u[u] - jlo_u[u], rp_u[u]
        for v in range(len(jlo_v)):
            cv, rv = jhi_v[v] - jlo_v[v], rp_v[v]
            frow = ru * Sv + cu * rv
            if normal == 0:
                row = rpn * S1 * S2 + cn * (ru * S2 + cu * rv)
                su, sv, base = cv, 1, jn * cu * cv
            elif normal == 1:
                row = ru * S1 * S2 + cu * (rpn * S2 + cn * rv)
                su, sv, base = cn * cv, 1, jn * cv
            else:
                row = ru * S1 * S2 + cu * (rv * S2 + cv * rpn)
                su, sv, base = cv * cn, cn, jn
            e = np.arange(cu * cv)
            out[frow + e] = row + base + (e // cv) * su + (e % cv) * sv
    return out


def add_face(values, kvs, axis, side, r):
    """``values[pos] += r``: one IEEE addition per touched entry (no two entries of one face share a position)."""
    pos = face_positions(kvs, axis, side)
    assert np.unique(pos).size == pos.size
    values[pos] = values[pos] + np.asarray(r, dtype=np.float64)
    return values


def canonical_pattern(kvs):
    """(indptr, indices) of the canonical CSR pattern of the tensor-product space `kvs`."""
    from pyiga_amd.assemble import _ml_nonzero
    I, J = _ml_nonzero(kvs, kvs, False)
    order = np.lexsort((J, I))
    I, J = I[order], J[order]
    n = int(np.prod([kv.numdofs for kv in kvs]))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=n))])
    return indptr.astype(np.int64), J.astype(np.int64)


def shifted_kron_pcg(A, b, kvs, K1, M1, shift, tol=1e-10, maxiter=500):
    """PCG on ``A x = b`` (dense, no fixed dof) with the fast-diagonalization preconditioner of ``sum_k K_k (x) M_rest`` whose
    per-axis eigenvalues are shifted by `shift` (``IGX_KRON_SUM`` with ``lam_k + shift``), or with Jacobi if `K1` is None.
    Returns (x, iterations)."""
    import scipy.linalg
    if K1 is None:
        dinv = 1.0 / np.diag(A)
        prec = lambda r: dinv * r
    else:
        ev = [scipy.linalg.eigh(K, M) for K, M in zip(K1, M1)]
        shape = tuple(K.shape[0] for K in K1)
        D = np.zeros(shape)
        for k, (lam, _) in enumerate(ev):
            D = D + (lam + shift).reshape([-1 if a == k else 1 for a in range(len(shape))])

        def kron_apply(mats, x):
            x = x.reshape(shape)
            for k, Mk in enumerate(mats):
                x = np.moveaxis(np.tensordot(Mk, x, axes=(1, k)), 0, k)
            return x
        prec = lambda r: kron_apply([U for _, U in ev], kron_apply([U.T for _, U in ev], r) / D).ravel()
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rz = r @ z
    r0 = np.linalg.norm(r)
    for it in range(1, maxiter + 1):
        Ap = A @ p
        a = rz / (p @ Ap)
        x += a * p
        r -= a * Ap
        if np.linalg.norm(r) <= tol * r0:
            return x, it
        z = prec(r)
        rz, old = r @ z, rz
        p = z + (rz / old) * p
    return x, maxiter + 1
