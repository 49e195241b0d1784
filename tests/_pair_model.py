"""Host model of a matrix over two spline spaces on one mesh (csrc/pair.hip), plain numpy: no GPU, no library load.

Two restatements, both written for any float type (float64, or long double for the device bound):

- ``physical_matrix``: from first principles -- dense collocation matrices of BOTH spaces (values and first derivatives of the
  active functions at the shared Gauss grid, scattered at each node's first active index), the inverse Jacobians, the Gauss
  weights times |det J| and the PHYSICAL coefficient table P[r][s] of  sum_rs P_rs D_r v D_s u  (D_0 = id, D_1.. = d/dx, d/dy
  [, d/dz]).  Independent of the device's field layout; compared with the reference's matrices.
- ``slot_matrix``: what ``pair_entry_value`` sums -- the patch's own quadrature fields (``DevicePatch.fields``), one per term
  of form_ab, times the parametric jets of u (trial tables) and v (test tables): value, magnitude (the same sum over absolute
  values) and number of Gauss points of every entry.  Acceptance of the device value, entry by entry:
      |dev - ref| <= (npts + C_KIND) 2**-53 mag
  (the bound of tests/_entries_model.py; it holds for every summation order).  C_KIND is counted from the source of
  pair_entry_value exactly as there from entry_value -- the expressions are the same: mass 2D ``((u0*u1)*(v0*v1))*f``: 3;
  mass 3D: 6; form, per term ``e += (F*du)*dv``: du and dv (1 product each in 2D, 2 in 3D), two products, one add: 5 in 2D, 7 in
  3D, times the number of terms (the first term sees every later add) -- ``_entries_model.c_kind``.

Pattern: row (i0, i1[, i2]) of the test space holds the columns [jlo_0, jhi_0) x [jlo_1, jhi_1) [x ..] of the trial space in
lexicographic order; [jlo_k, jhi_k) are the trial functions of axis k whose mesh support meets that of test function i_k.
"""
import numpy as np

LD = np.longdouble


def ranges(kv_trial, kv_test):
    """(jlo, jhi) per test dof of one axis, from the two knot vectors' mesh supports."""
    su = np.asarray(kv_trial.mesh_support_idx_all(), dtype=np.int64)
    sv = np.asarray(kv_test.mesh_support_idx_all(), dtype=np.int64)
    jlo = np.searchsorted(su[:, 1], sv[:, 0], side='right')            # first j with mshi[j] > mslo[i]
    jhi = np.searchsorted(su[:, 0], sv[:, 1], side='left')             # first j with mslo[j] >= mshi[i]
    return jlo, jhi


def pattern(kvs_trial, kvs_test):
    """(indptr, indices, longest row) of the canonical CSR."""
    rng = [ranges(a, b) for a, b in zip(kvs_trial, kvs_test)]
    nu = [int(kv.numdofs) for kv in kvs_trial]
    nv = [int(kv.numdofs) for kv in kvs_test]
    rows = []
    for I in range(int(np.prod(nv))):
        i = np.unravel_index(I, nv)
        cols = np.zeros(1, dtype=np.int64)
        for k, ik in enumerate(i):
            cols = (cols[:, None] * nu[k] + np.arange(rng[k][0][ik], rng[k][1][ik])[None, :]).ravel()
        rows.append(cols)
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    maxrow = int(np.prod([int((hi - lo).max()) for lo, hi in rng]))
    return indptr, np.concatenate(rows), maxrow


def npts_matrix(kvs_trial, kvs_test, q):
    """Gauss points of the support intersection of every (test row, trial column) pair; 0: disjoint supports."""
    out = None
    for a, b in zip(kvs_trial, kvs_test):
        su = np.asarray(a.mesh_support_idx_all(), dtype=np.int64)
        sv = np.asarray(b.mesh_support_idx_all(), dtype=np.int64)
        ov = np.minimum(sv[:, None, 1], su[None, :, 1]) - np.maximum(sv[:, None, 0], su[None, :, 0])
        ov = np.maximum(ov, 0) * q
        out = ov if out is None else (out[:, None, :, None] * ov[None, :, None, :]).reshape(out.shape[0] * ov.shape[0], -1)
    return out


def dense_colloc(kv, first, vals, dtype=np.float64):
    """[B_value, B_derivative], each (G, numdofs): vals (>= 2, p + 1, G) as ``active_deriv`` returns them, scattered at the
    first active index of every node."""
    G, N, P = vals.shape[2], int(kv.numdofs), vals.shape[1]
    out = np.zeros((2, G, N), dtype=dtype)
    cols = np.asarray(first)[:, None] + np.arange(P)[None, :]
    keep = cols < N                                # (only a mutated table can leave the space)
    g = np.broadcast_to(np.arange(G)[:, None], cols.shape)
    for s in range(2):
        out[s][g[keep], cols[keep]] = np.moveaxis(np.asarray(vals[s], dtype=dtype), 0, 1)[keep]
    return out


def _jet_products(B, slots):
    """prod_k B[k][slots[k]][g_k, i_k] -> (G0, .., N0, ..) flattened to (G0, .., N)."""
    d = len(B)
    letters_g, letters_i = 'abc'[:d], 'ijk'[:d]
    spec = ','.join(letters_g[k] + letters_i[k] for k in range(d)) + '->' + letters_g + letters_i
    T = np.einsum(spec, *[B[k][slots[k]] for k in range(d)])
    return T.reshape(T.shape[:d] + (-1,))


def jet_slots(dim, c):
    """Slots per grid axis of jet index c: the derivative c >= 1 acts on grid axis dim - c (x = the LAST grid axis)."""
    return tuple(1 if c >= 1 and k == dim - c else 0 for k in range(dim))


def physical_matrix(Bu, Bv, W, JI, table, dtype=np.float64):
    """Dense (test dofs, trial dofs) matrix of  sum_g W sum_rs P_rs D_r v D_s u.

    Bu, Bv: per axis dense_colloc of the trial / test space; W: (G..) weights times |det J|; JI: (G.., d, d) inverse Jacobian,
    JI[.., a, r] = d xi_a / d x_r with the parametric directions a in (x, y, z) order; table: (d+1) x (d+1) of arrays over the
    grid, numbers or None."""
    d = len(Bu)
    Gs = W.shape

    def phys_jets(B):
        par = [_jet_products(B, jet_slots(d, c)) for c in range(d + 1)]          # parametric jets, (G.., N)
        out = [par[0]]
        for r in range(d):
            out.append(sum(np.asarray(JI[..., a, r], dtype=dtype)[..., None] * par[1 + a] for a in range(d)))
        return out
    Ju, Jv = phys_jets(Bu), phys_jets(Bv)
    A = np.zeros((Jv[0].shape[-1], Ju[0].shape[-1]), dtype=dtype)
    ng = int(np.prod(Gs))
    for r in range(d + 1):
        for s in range(d + 1):
            if table[r][s] is None:
                continue
            c = (np.asarray(W, dtype=dtype) * np.asarray(np.broadcast_to(table[r][s], Gs), dtype=dtype)).reshape(ng)
            A += (Jv[r].reshape(ng, -1) * c[:, None]).T @ Ju[s].reshape(ng, -1)
    return A


def slot_matrix(Bu, Bv, fields, terms):
    """(value, magnitude), dense (test dofs, trial dofs), long double: sum over the terms (field, slots of u, slots of v) of
    F_t * prod_k u_k[slot] * prod_k v_k[slot] over all Gauss points (outside the support intersection the products vanish)."""
    Gs = fields.shape[1:]
    ng = int(np.prod(Gs))
    val = mag = None
    for t, us, vs in terms:
        F = np.asarray(fields[t], dtype=LD).reshape(ng)
        U = _jet_products(Bu, us).reshape(ng, -1)
        V = _jet_products(Bv, vs).reshape(ng, -1)
        a = (V * F[:, None]).T @ U
        m = (abs(V) * abs(F)[:, None]).T @ abs(U)
        val, mag = (a, m) if val is None else (val + a, mag + m)
    return val, mag


def rel_maxdiff(A, B):
    """max |A - B| / max |B| of dense arrays."""
    return float(abs(np.asarray(A) - np.asarray(B)).max() / abs(np.asarray(B)).max())
