#!/usr/bin/env python3
"""Generate tests/golden/arith_fe_{D2Q9,D3Q19}.npz from the reference's sympy objects of the free-energy binary fluid
(sym_equilibrium.free_energy_equilibrium_fluid / free_energy_equilibrium_order_param with the weight tables that
lb_binary.LBBinaryFluidFreeEnergy._prepare_symbols builds).

Runs only where the reference is importable (tools/ref_shim.py); the fixtures are data -- inputs and expected values --
and nothing in tests/ or the product reads the reference at run time.  Every expected value is the reference's own
expression object evaluated at 30 digits and rounded to float64.

    PYTHONPATH=tools python tools/capture_fe.py

Per lattice:
    wi, wxx, wyy, wzz, wxy, wyz, wxz      [Q - 1]            the weight tables
    A, kappa, Gamma, tau_a, tau_b         scalars            the parameters the states were evaluated with
    rho, phi, lap, v, grad                [n], [n, dim]      states: |v| <= 0.1, phi in [-1.3, 1.3]; grad = 0 in the
                                                             first half (the uniform boxes of the GPU tests)
    feq_fluid, feq_order                  [n, Q]             the two equilibria on them (local variables pb / mu first)
    tau0                                  [n]                relaxation_common.mako:156-163 on phi, in exact arithmetic
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: F401  (installs import stubs, puts the reference on sys.path)

import numpy as np
import sympy

from sailfish import lb_binary, sym, sym_equilibrium  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
PARAMS = dict(A=0.04, kappa=0.03, Gamma=0.6, tau_a=1.3, tau_b=0.8)
TABLES = ('wi', 'wxx', 'wyy', 'wzz', 'wxy', 'wyz', 'wxz')


def prepare(grid):
    """The reference's symbols and weight tables for `grid`, set up by its own _prepare_symbols()."""
    sim = object.__new__(lb_binary.LBBinaryFluidFreeEnergy)
    sim.S = sym.S
    sim.grids = [grid]
    sim._prepare_symbols()
    return sim.S


def _evalf(expr, values):
    if not isinstance(expr, sympy.Basic):
        return sympy.Float(expr, 30)
    subs = {}
    for s in expr.free_symbols:
        if s not in values:
            raise KeyError('unbound symbol %s' % s)
        subs[s] = sympy.Float(values[s], 30)
    return expr.subs(subs).evalf(30)


def equilibrium(eq, values):
    values = dict(values)
    for lv in eq.local_vars:
        values[lv.lhs] = _evalf(lv.rhs, values)
    return np.array([float(_evalf(e, values)) for e in eq.expression])


def exact_tau0(phi, tau_a, tau_b):
    r = sympy.Rational
    phi, tau_a, tau_b = r(repr(float(phi))), r(repr(tau_a)), r(repr(tau_b))
    if phi < -1:
        return float(tau_b)
    if phi > 1:
        return float(tau_a)
    return float(tau_b + (phi + 1) * (tau_a - tau_b) / 2)


def capture(grid, rng):
    S = prepare(grid)
    out = dict((name, np.array([float(w) for w in getattr(S, name)][:grid.Q - 1])) for name in TABLES)
    out.update(PARAMS)
    eq_f = sym_equilibrium.free_energy_equilibrium_fluid(grid, None)
    eq_o = sym_equilibrium.free_energy_equilibrium_order_param(grid, None)
    n, dim = 48, grid.dim
    rho = rng.uniform(0.8, 1.2, n)
    phi = rng.uniform(-1.3, 1.3, n)
    phi[:4] = [-1.25, 1.25, -1.0, 1.0]
    lap = rng.uniform(-0.2, 0.2, n)
    v = rng.uniform(-1.0, 1.0, (n, dim))
    v = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.0, 0.1, n)[:, None]
    v[0] = 0.0
    grad = rng.uniform(-0.3, 0.3, (n, dim))
    grad[:n // 2] = 0.0
    assert (phi < -1).sum() >= 3 and (phi > 1).sum() >= 3
    grads = [S.g1d1m0x, S.g1d1m0y, S.g1d1m0z]
    ff, fo = [], []
    for k in range(n):
        values = {S.rho: rho[k], S.phi: phi[k], S.g1d2m0: lap[k], S.A: PARAMS['A'], S.kappa: PARAMS['kappa'],
                  S.Gamma: PARAMS['Gamma'], S.visc: 0.1}
        for d in range(3):
            values[grads[d]] = grad[k, d] if d < dim else 0.0
        for d in range(dim):
            values[grid.v[d]] = v[k, d]
            values[S.grad0[d]] = 0.0
        ff.append(equilibrium(eq_f, values))
        fo.append(equilibrium(eq_o, values))
    out.update(rho=rho, phi=phi, lap=lap, v=v, grad=grad, feq_fluid=np.array(ff), feq_order=np.array(fo),
               tau0=np.array([exact_tau0(p, PARAMS['tau_a'], PARAMS['tau_b']) for p in phi]))
    return out


if __name__ == '__main__':
    for grid in (sym.D2Q9, sym.D3Q19):
        rng = np.random.RandomState(31000 + grid.Q)
        data = capture(grid, rng)
        path = os.path.join(OUT, 'arith_fe_%s.npz' % grid.__name__)
        np.savez(path, **data)
        print(path, {k: np.shape(v) for k, v in data.items()})
