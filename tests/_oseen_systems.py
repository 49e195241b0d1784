"""The Oseen problems of the device tests of the GMRES solver, built with this package as the reference's solve-navier-stokes
notebook builds each of its linear systems: the Stokes problems of _saddle_systems.py ('stokes', 'stokes3') with the rotating winds
and the viscosity of golden_oseen.npz ('oseen2', 'oseen3').  Needs the device."""
from pyiga_amd import solvers

from _saddle_systems import problem as _problem


def wind2(x, y):
    return (-y, x)


def wind3(x, y, z):
    return (-y, x, 0.25 + 0.0 * z)


BASE = {'oseen2': 'stokes', 'oseen3': 'stokes3'}


def system(name, nu=None, which='pinned', **kw):
    """OseenSystem of the golden case `name` with viscosity `nu`, or -- 'stokes' / 'stokes3' -- of the Stokes problem
    (convection=None, viscosity 1).  Returns (system, number of velocity unknowns)."""
    base = BASE.get(name, name)
    kvs_u, kvs_p, geo, bcs, nv = _problem(base)
    if which == 'unpinned':
        bcs = (bcs[0][:-1], bcs[1][:-1])
    if name in BASE:
        kw = dict(dict(viscosity=nu, w=wind2 if name == 'oseen2' else wind3), **kw)
    else:
        kw = dict(dict(convection=None), **kw)
    return solvers.OseenSystem((kvs_u, kvs_p), geo, bcs, **kw), nv
