#!/usr/bin/env python3
"""Generate the fixtures of the D3Q15 / D3Q27 lattices from the reference's own objects:

    tests/golden/lattices_q15_q27.json        the tables of sym.D3Q15 / sym.D3Q27 and what sym.get_prop_dists,
                                              get_interblock_dists and get_missing_dists make of them
    tests/golden/arith_lat_{D3Q15,D3Q27}.npz  states and the values of the reference's expression objects at them

Runs only where the reference is importable (tools/ref_shim.py); the fixtures are data -- inputs and expected values --
and nothing in tests/ or the product reads the reference at run time.  Every expected value is the reference's own sympy
expression evaluated at 30 digits and rounded to float64.

    PYTHONPATH=tools python tools/capture_lattices.py

Per lattice (n states):
    rho, v, accel            [n], [n, 3], [n, 3]   rho in [0.8, 1.2], |v| <= 0.1 (state 0: at rest), accelerations
    visc, tau                scalars               the viscosity of the Guo prefactor and sym.relaxation_time of it
    feq, feq_incompressible  [n, Q]                sym_equilibrium.bgk_equilibrium(grid, cfg).expression
    guo                      [n, Q]                sym_force.guo_external_force x guo_external_force_pref (at rho, v as given)
    edm                      [n, Q]                sym_force.edm_shift_velocity of the compressible equilibrium: feq_i(rho, v + a)
    f                        [n, Q]                populations (the equilibrium, perturbed by up to 5 %)
    mom_rho, mom_v, mom_v_incompressible  [n], [n, 3], [n, 3]   sym.ex_rho / sym.ex_velocity of f
"""
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: F401  (installs import stubs, puts the reference on sys.path)

import numpy as np
import sympy

from sailfish import sym, sym_equilibrium, sym_force  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
VISC = 0.02


class _Cfg(object):
    def __init__(self, incompressible=False):
        self.incompressible = incompressible
        self.minimize_roundoff = False


def _evalf(expr, subs):
    if isinstance(expr, (int, float)):
        return float(expr)
    m = {}
    for s in expr.free_symbols:
        if s.name not in subs:
            raise KeyError('unbound symbol %s in %s' % (s.name, expr))
        m[s] = sympy.Float(subs[s.name], 30)
    return float(expr.subs(m).evalf(30))


def lattice_tables(grid):
    dim = grid.dim
    t = {
        'name': grid.__name__, 'dim': dim, 'Q': grid.Q,
        'basis': [[int(c) for c in e] for e in grid.basis],
        'weights_num': [int(w.p) for w in grid.weights],
        'weights_den': [int(w.q) for w in grid.weights],
        'idx_name': list(grid.idx_name),
        'idx_opposite': [int(i) for i in grid.idx_opposite],
        'dir2vecidx': {str(k): int(v) for k, v in grid.dir2vecidx.items()},
        'prop_dists': {('%d_%d' % (axis, d)): [int(i) for i in sym.get_prop_dists(grid, d, axis)]
                       for axis in range(dim) for d in (-1, 0, 1)},
        'missing_dists': {str(o): [int(i) for i in sym.get_missing_dists(grid, o)] for o in range(1, 2 * dim + 1)},
        'has_mrt': bool(hasattr(grid, 'mrt_matrix')),
    }
    ib = {}
    for d in itertools.product((-1, 0, 1), repeat=dim):
        if any(d):
            ib[','.join(str(c) for c in d)] = {
                'normal': [int(i) for i in sym.get_interblock_dists(grid, d)],
                'opposite': [int(i) for i in sym.get_interblock_dists(grid, d, opposite=True)]}
    t['interblock_dists'] = ib
    return t


def arithmetic(grid, rng, n=32):
    dim, Q = grid.dim, grid.Q
    rho = rng.uniform(0.8, 1.2, n)
    v = rng.uniform(-1.0, 1.0, (n, dim))
    v = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.0, 0.1, n)[:, None]
    v[0] = 0.0
    accel = rng.uniform(-1e-3, 1e-3, (n, dim))
    tau = float(sym.relaxation_time(VISC))
    cfg, cfg_inc = _Cfg(), _Cfg(incompressible=True)
    eq = sym_equilibrium.bgk_equilibrium(grid, cfg).expression
    eq_inc = sym_equilibrium.bgk_equilibrium(grid, cfg_inc).expression
    guo = sym_force.guo_external_force(grid, grid_num=0)
    pref_e = sym_force.guo_external_force_pref(grid, cfg, grid_num=0)
    edm = sym_force.edm_shift_velocity(eq, grid, 0)
    ex_rho = sym.ex_rho(grid, 'fi', False)
    ex_v = [sym.ex_velocity(grid, 'fi', d, cfg) for d in range(dim)]
    ex_v_inc = [sym.ex_velocity(grid, 'fi', d, cfg_inc) for d in range(dim)]
    out = dict(rho=rho, v=v, accel=accel, visc=np.float64(VISC), tau=np.float64(tau))
    feq, feq_inc, g, e = (np.zeros((n, Q)) for _ in range(4))
    for k in range(n):
        subs = {'g0m0': float(rho[k]), 'rho': float(rho[k]), 'rho0': float(rho[k]), 'tau0': tau}
        for j, c in enumerate('xyz'):
            subs['g0m1' + c] = float(v[k, j])
            subs['g0ea' + c] = float(accel[k, j])
        subs_inc = dict(subs, rho0=1.0)
        subs['pref'] = _evalf(pref_e, subs)
        for i in range(Q):
            feq[k, i] = _evalf(eq[i], subs)
            feq_inc[k, i] = _evalf(eq_inc[i], subs_inc)
            g[k, i] = _evalf(guo[i], subs)
            e[k, i] = _evalf(edm[i], subs)
    f = feq * (1.0 + rng.uniform(-0.05, 0.05, (n, Q)))
    m_rho, m_v, m_v_inc = np.zeros(n), np.zeros((n, dim)), np.zeros((n, dim))
    for k in range(n):
        subs = {'fi->%s' % name: float(x) for name, x in zip(grid.idx_name, f[k])}
        m_rho[k] = _evalf(ex_rho, subs)
        subs.update({'g0m0': m_rho[k], 'rho': m_rho[k], 'rho0': m_rho[k]})
        for d in range(dim):
            m_v[k, d] = _evalf(ex_v[d], subs)
            m_v_inc[k, d] = _evalf(ex_v_inc[d], dict(subs, rho0=1.0))
    out.update(feq=feq, feq_incompressible=feq_inc, guo=g, edm=e, f=f, mom_rho=m_rho, mom_v=m_v, mom_v_incompressible=m_v_inc)
    return out


if __name__ == '__main__':
    grids = (sym.D3Q15, sym.D3Q27)
    path = os.path.join(OUT, 'lattices_q15_q27.json')
    with open(path, 'w') as fh:
        json.dump({g.__name__: lattice_tables(g) for g in grids}, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(path)
    for grid in grids:
        data = arithmetic(grid, np.random.RandomState(41000 + grid.Q))
        path = os.path.join(OUT, 'arith_lat_%s.npz' % grid.__name__)
        np.savez(path, **data)
        print(path, {k: np.shape(x) for k, x in data.items()})
