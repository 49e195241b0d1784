"""numpy model of the device BiCGStab (igx_solver_solve with IGX_METHOD_BICGSTAB, pyiga_amd/csrc/solve.hip): the same
right-preconditioned "Templates" iteration, the same stopping rule ||r|| <= tol ||b||, the same freeze (the s test and an omega
breakdown keep the half step) and the same breakdown rule: rho = r^.r counts as zero when it has cancelled to below EPS_RHO times
the sum of the magnitudes of its terms (a restart with r^ = p = r; a second one right after it stops), and r^.v when the step
alpha v would exceed ||r|| / EPS_ALPHA."""
import numpy as np

EPS_RHO = np.finfo(float).eps ** 2     # breakdown: |rho| <= EPS_RHO sum |r^_i r_i|   (BICG_EPS_RHO)
EPS_ALPHA = 1e-13                       #            EPS_ALPHA |alpha| ||v|| > ||r||  (BICG_EPS_ALPHA)
REASONS = {0: None, 1: 'rho', 2: 'alpha', 3: 'omega', 4: 'nonfinite'}


def bicgstab(A, b, tol=1e-8, maxiter=1000, M=None, x0=None, callback=None):
    """Solves A x = b.  `M(r)`: the preconditioner (None: identity).  `callback(x)` after every x update.  Returns x and a dict
    with iterations, converged, relres and breakdown (None or 'rho' / 'alpha' / 'omega' / 'nonfinite')."""
    A_ = (lambda y: A @ y)
    M_ = M if M is not None else (lambda y: y.copy())
    b = np.asarray(b, dtype=np.float64)
    bnorm = np.linalg.norm(b)
    stop = tol * bnorm
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A_(x) if x0 is not None else b.copy()
    rh = r.copy()
    p = np.zeros_like(b)
    v = np.zeros_like(b)
    st = dict(it=0, done=False, last=False, conv=False, reason=0, rho=0.0, rho_old=0.0, alpha=0.0, omega=0.0, beta=0.0, rr=0.0,
              restart=False, restart_it=None, restarts=0)

    def halt(conv, reason):
        st.update(done=True, conv=conv)
        if reason:
            st['reason'] = reason

    def fin_rho(rr, rho, arho):
        st['rr'] = rr
        if st['last']:
            st['done'] = True
            return
        if not (np.isfinite(rr) and np.isfinite(rho)):
            return halt(False, 4)
        if np.sqrt(rr) <= stop:
            return halt(True, 0)
        if abs(rho) <= EPS_RHO * arho:
            if st['restart_it'] is not None and st['restart_it'] == st['it'] - 1:
                return halt(False, 1)
            st.update(restart=True, restart_it=st['it'], restarts=st['restarts'] + 1, beta=0.0, rho=rr, rho_old=rr)
            return
        beta = (rho / st['rho_old']) * (st['alpha'] / st['omega']) if st['it'] > 0 else 0.0
        if not np.isfinite(beta):
            return halt(False, 4)
        st.update(beta=beta, rho=rho, rho_old=rho)

    rr = float(r @ r)
    fin_rho(rr, rr, rr)
    with np.errstate(all='ignore'):
        for _ in range(maxiter):
            if st['done']:
                break
            if st['restart']:
                p = r.copy()
                rh = r.copy()
            else:
                p = r + st['beta'] * (p - st['omega'] * v)
            ph = M_(p)
            v = A_(ph)
            rv = float(rh @ v)
            st['it'] += 1
            st['restart'] = False
            alpha = st['rho'] / rv
            if not (np.isfinite(rv) and np.isfinite(alpha)):
                halt(False, 2 if rv == 0.0 else 4)
                break
            st['alpha'] = alpha
            s = r - alpha * v
            ss, vv = float(s @ s), float(v @ v)
            if not (np.isfinite(ss) and np.isfinite(vv)):
                halt(False, 4)
                break
            if EPS_ALPHA * abs(alpha) * np.sqrt(vv) > np.sqrt(st['rr']):
                halt(False, 2)
                break
            if np.sqrt(ss) <= stop:
                st.update(last=True, conv=True)
            sh = M_(s)
            t = A_(sh)
            ts, tt = float(t @ s), float(t @ t)
            if st['last']:
                omega = 0.0
            else:
                omega = ts / tt
                if not np.isfinite(omega) or omega == 0.0:
                    st.update(last=True, reason=3 if np.isfinite(ts) and np.isfinite(tt) else 4)
                    omega = 0.0
            st['omega'] = omega
            x = x + alpha * ph
            r = s
            if omega != 0.0:
                x = x + omega * sh
                r = s - omega * t
            if callback is not None:
                callback(x)
            fin_rho(float(r @ r), float(rh @ r), float(np.abs(rh) @ np.abs(r)))
    return x, dict(iterations=st['it'], converged=bool(st['conv']), relres=np.sqrt(st['rr']) / bnorm if bnorm > 0 else 0.0,
                   breakdown=REASONS[st['reason']], restarts=st['restarts'])
