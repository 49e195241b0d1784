"""Host model of the multipatch pattern and scatter (pyiga_amd/csrc/multipatch.hip; numpy / scipy only, no device).

Input: the local CSR pattern of every patch (canonical: sorted unique columns per row), the maps ``l2g_p`` and ``nglobal``.
Output: everything the twelve kernels of multipatch.hip produce, computed from the definitions of DESIGN.md section 11 and
include/igx.h -- not from the kernels:

- per global row r: ``contrib[r]`` (local rows mapped to r), the raw length ``L[r]`` (their entries, duplicates counted) and
  the sorted unique mapped columns; from these ``indptr``, ``indices``, ``nnz``;
- ``injective``: no map sends two local dofs of one patch to one global dof;
- the class of every local row (ATOMIC everywhere when not injective; else RMW where contrib > 1; else DIRECT where the
  mapped columns increase strictly, so that the global row is the local row entry for entry; else STORE), the entries per
  class, ``delta`` of the direct rows and the global position of every local entry;
- ``zero_from``: ``indptr[r0]`` where r0 splits the rows into contrib == 1 before it and contrib != 1 from it on (r0 = G when
  no row differs from 1); 0 when there is no such split or a map is not injective;
- the sums: ``sum_values`` in float64, patch after patch with ``out[pos] += v`` (the device's bits for injective maps), and
  ``sum_values_ld`` in long double with the number of terms and the sum of moduli per position; the same pair for vectors.

``staged_pattern`` is a second, stage-by-stage host build (scan, per-row sort, de-duplication, shortcut) whose stages can be
replaced: tests/test_multipatch_coverage_cpu.py plugs deliberately wrong stages in to show that the case table tells a wrong
kernel from a right one.  With the default stages it equals the model.
"""
import numpy as np

DIRECT, STORE, RMW, ATOMIC = 0, 1, 2, 3          # the order of igx_multipatch_info.entries
CLASS_NAMES = ('direct', 'store', 'rmw', 'atomic')


class Model:
    def __init__(self, patterns, l2g, nglobal):
        G = self.G = int(nglobal)
        self.np = len(patterns)
        self.l2g = [np.asarray(m, dtype=np.int64) for m in l2g]
        self.lindptr = [np.asarray(S.indptr, dtype=np.int64) for S in patterns]
        self.lindices = [np.asarray(S.indices, dtype=np.int64) for S in patterns]
        for m, ip in zip(self.l2g, self.lindptr):
            assert m.size == ip.size - 1 and m.min() >= 0 and m.max() < G
        self.lrows = [np.repeat(np.arange(ip.size - 1), np.diff(ip)) for ip in self.lindptr]
        self.grow = [m[r] for m, r in zip(self.l2g, self.lrows)]          # global row of every local entry
        self.gcol = [m[c] for m, c in zip(self.l2g, self.lindices)]       # global column of every local entry
        self.contrib = np.bincount(np.concatenate(self.l2g), minlength=G)
        self.L = np.bincount(np.concatenate(self.grow), minlength=G)
        # the pattern: the set of (row, column) pairs in row-major order
        keys = [r * G + c for r, c in zip(self.grow, self.gcol)]
        ukeys = np.unique(np.concatenate(keys))
        self.nnz = int(ukeys.size)
        self.indices = (ukeys % G).astype(np.int32)
        self.ucnt = np.bincount(ukeys // G, minlength=G)
        self.indptr = np.concatenate(([0], np.cumsum(self.ucnt))).astype(np.int64)
        self.pos = [np.searchsorted(ukeys, k) for k in keys]
        for k, q in zip(keys, self.pos):
            assert np.array_equal(ukeys[q], k)
        self.injective = all(np.unique(m).size == m.size for m in self.l2g)
        # classes
        self.increasing = []          # per patch, per local row: the mapped columns increase strictly
        self.cls = []
        self.delta = []               # per patch, per local row: indptr[r] - local indptr[i] (meaningful for DIRECT rows)
        self.entries = [0, 0, 0, 0]
        for p in range(self.np):
            n = self.l2g[p].size
            rows, gc = self.lrows[p], self.gcol[p]
            bad = (rows[1:] == rows[:-1]) & (gc[1:] <= gc[:-1])
            inc = np.bincount(rows[1:][bad], minlength=n) == 0
            c = self.contrib[self.l2g[p]]
            cls = np.where(c > 1, RMW, np.where(inc, DIRECT, STORE))
            if not self.injective:
                cls = np.full(n, ATOMIC)
            self.increasing.append(inc)
            self.cls.append(cls)
            self.delta.append(self.indptr[self.l2g[p]] - self.lindptr[p][:-1])
            lens = np.diff(self.lindptr[p])
            for k in range(4):
                self.entries[k] += int(lens[cls == k].sum())
        # a global row is left unsorted when one local row reaches it and that row's mapped columns increase strictly
        self.as_is = np.zeros(G, dtype=bool)
        for p in range(self.np):
            self.as_is[self.l2g[p][self.increasing[p]]] = True
        self.as_is &= self.contrib == 1
        # zero_from
        self.r0 = self.split_row(self.contrib)
        self.vzero_from = self.r0 if self.injective and self.r0 is not None else 0
        self.zero_from = int(self.indptr[self.vzero_from])

    @staticmethod
    def split_row(contrib):
        """r0 with contrib == 1 on [0, r0) and contrib != 1 on [r0, G); None when the rows do not split that way."""
        other = np.flatnonzero(contrib != 1)
        if other.size == 0:
            return int(contrib.size)
        r0 = int(other[0])
        return r0 if other.size == contrib.size - r0 else None

    def info(self):
        return dict(npatches=self.np, injective=int(self.injective), nrows=self.G, nnz=self.nnz,
                    entries=tuple(self.entries), zero_from=self.zero_from)

    # --- sums --------------------------------------------------------------------------------
    def _sum(self, where, vals, size, dtype):
        out = np.zeros(size, dtype=dtype)
        for q, v in zip(where, vals):
            v = np.asarray(v, dtype=dtype)
            if self.injective:
                out[q] += v                   # no two entries of one patch collide: the vectorised add is the sequential one
            else:
                np.add.at(out, q, v)
        return out

    def _terms(self, where, vals, size):
        m = np.zeros(size, dtype=np.int64)
        sabs = np.zeros(size, dtype=np.longdouble)
        for q, v in zip(where, vals):
            np.add.at(m, q, 1)
            np.add.at(sabs, q, np.abs(np.asarray(v, dtype=np.longdouble)))
        return m, sabs

    def sum_values(self, vals):
        """float64, patch after patch in patch order, out[pos] += v within a patch."""
        return self._sum(self.pos, vals, self.nnz, np.float64)

    def sum_values_ld(self, vals):
        """(the sum in long double, the number of terms per position, the sum of their moduli)."""
        return (self._sum(self.pos, vals, self.nnz, np.longdouble),) + self._terms(self.pos, vals, self.nnz)

    def sum_vector(self, bs):
        return self._sum(self.l2g, bs, self.G, np.float64)

    def sum_vector_ld(self, bs):
        return (self._sum(self.l2g, bs, self.G, np.longdouble),) + self._terms(self.l2g, bs, self.G)

    def dense(self, vals):
        """sum_p X_p A_p X_p^T as a dense float64 matrix through scipy (small cases): the check of the model itself."""
        import scipy.sparse
        A = np.zeros((self.G, self.G))
        for p in range(self.np):
            n = self.l2g[p].size
            X = scipy.sparse.csr_matrix((np.ones(n), (self.l2g[p], np.arange(n))), shape=(self.G, n))
            Ap = scipy.sparse.csr_matrix((np.asarray(vals[p], dtype=np.float64), self.lindices[p], self.lindptr[p]), shape=(n, n))
            A += (X @ Ap @ X.T).toarray()
        return A


def sum_bound(m, sabs):
    """|float64 sum in any order - long double sum| <= gamma_{m-1} sum|a| + (m - 1) 2^-64 sum|a|, gamma_k = k u / (1 - k u),
    u = 2^-53: the bound of recursive summation (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) plus the
    same first-order bound for the long double reference itself."""
    u = np.longdouble(2.0) ** -53
    k = np.maximum(m - 1, 0).astype(np.longdouble)
    return (k * u / (1 - k * u) + k * np.longdouble(2.0) ** -64) * sabs


# ---------------------------------------------------------------------------------------------
# the staged build and its replaceable stages
def scan_exact(x, chunk):
    return np.concatenate(([0], np.cumsum(x, dtype=np.int64)))


def sort_exact(raw):
    return np.sort(raw, kind='stable')


def dedup_exact(s, wave):
    keep = np.ones(s.size, dtype=bool)
    keep[1:] = s[1:] != s[:-1]
    return s[keep]


def shortcut_exact(raw):
    """A row one local row reaches is left as it is when its columns increase strictly."""
    return bool((raw[1:] > raw[:-1]).all())


def zero_row_exact(contrib):
    return Model.split_row(contrib)


DEFAULT_STAGES = dict(scan=scan_exact, sort_short=sort_exact, sort_long=sort_exact, dedup=dedup_exact,
                      shortcut=shortcut_exact, zero_row=zero_row_exact, rmw_adds=True)


def staged_pattern(model, consts, rows=True, **stages):
    """(indptr, indices, zero_from, n_long) built stage by stage as DESIGN.md section 11 lists them: raw rows in fill order (patch
    after patch, local row after local row), per-row shortcut / sort / de-duplication, scan of the unique counts, compaction.
    ``rows=False`` takes the unique rows from the model (for cases too large for a Python loop over their rows; the scans and
    the zero rule still run)."""
    st = dict(DEFAULT_STAGES, **stages)
    G = model.G
    chunk = consts['SCAN_BLOCK'] * consts['SCAN_BLOCK'] * consts['SCAN_ITEMS']     # inputs one trip of the tile-sum scan covers
    upoff = st['scan'](model.L, chunk)
    n_long = 0
    if rows:
        grow = np.concatenate(model.grow)
        gcol = np.concatenate(model.gcol)
        order = np.argsort(grow, kind='stable')
        raw_all = gcol[order]
        true_off = np.concatenate(([0], np.cumsum(model.L)))
        uniq = []
        for r in range(G):
            L = int(model.L[r])
            raw = raw_all[true_off[r]:true_off[r] + L]
            if model.contrib[r] == 1 and st['shortcut'](raw):
                uniq.append(raw)
            elif L > consts['SORT_TILE']:
                n_long += 1
                uniq.append(dedup_exact(st['sort_long'](raw), consts['WAVE']))
            else:
                uniq.append(st['dedup'](st['sort_short'](raw), consts['WAVE']))
        ucnt = np.array([u.size for u in uniq], dtype=np.int64)
        cols = np.concatenate(uniq) if uniq else np.zeros(0, dtype=np.int64)
    else:
        ucnt, cols = model.ucnt, model.indices.astype(np.int64)
    gptr = st['scan'](ucnt, chunk)
    # compaction: row r goes to [gptr[r], gptr[r] + ucnt[r])
    indices = np.full(max(int(gptr[-1]), int((gptr[:-1] + ucnt).max(initial=0))), -1, dtype=np.int64)
    true_ptr = np.concatenate(([0], np.cumsum(ucnt)))
    dst = np.repeat(gptr[:-1] - true_ptr[:-1], ucnt) + np.arange(cols.size)
    indices[dst] = cols
    indices = indices[:int(gptr[-1])]
    r0 = st['zero_row'](model.contrib)
    zero_from = int(gptr[r0]) if model.injective and r0 is not None else 0
    return gptr, indices, zero_from, n_long


def staged_values(model, vals, rmw_adds=True):
    """The scatter by classes: DIRECT and STORE rows store, RMW rows add (or store, when `rmw_adds` is off), ATOMIC rows add."""
    out = np.zeros(model.nnz)
    for p in range(model.np):
        cls_e = model.cls[p][model.lrows[p]]
        v = np.asarray(vals[p], dtype=np.float64)
        st = cls_e <= STORE
        out[model.pos[p][st]] = v[st]
        rm = cls_e == RMW
        if rmw_adds:
            out[model.pos[p][rm]] += v[rm]
        else:
            out[model.pos[p][rm]] = v[rm]
        at = cls_e == ATOMIC
        np.add.at(out, model.pos[p][at], v[at])
    return out
