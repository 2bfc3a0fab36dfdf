#!/usr/bin/env python3
"""Generate tests/golden/arith_sc3_{D2Q9,D3Q19}.npz from the reference's own objects of the ternary Shan-Chen mixture
(lb_ternary.LBTernaryFluidShanChen: its constants() and force couplings, its three equilibria; sym_force.guo_external_force
x guo_external_force_pref for grid_num = 0, 1, 2; the two pseudopotentials of sym.SHAN_CHEN_POTENTIALS).

Runs only where the reference is importable (tools/ref_shim.py); the fixtures are data -- inputs and expected values --
and nothing in tests/ or the product reads the reference at run time.  Every expected value is the reference's own
expression object evaluated at 30 digits and rounded to float64.

    PYTHONPATH=tools python tools/capture_sc3.py

The class is instantiated with a plain namespace as its config (grid, the six couplings, the relaxation times); nothing of
the reference's controller or code generation runs.

Per lattice:
    coupling_names, coupling_values   [9]               constants() restricted to the G.. names, in sorted order
    force_couplings                   [9, 2], names [9] the (lattice, field) pairs and their constants in iteration order
    G, tau                            [6], [3]          the option values: G11 G12 G13 G22 G23 G33; tau(visc) tau_phi tau_theta
    dens, v, accel                    [n, 3], [n, dim], [n, 3, dim]   states: |v| <= 0.1, positive densities
    feq                               [n, 3, Q]         the three equilibria (rho, phi, theta)
    guo                               [n, 3, Q]         guo_external_force x guo_external_force_pref per grid_num
    psi_rho, psi_linear, psi_classic  [m]               the pseudopotentials
"""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: F401  (installs import stubs, puts the reference on sys.path)

import numpy as np
import sympy

from sailfish import lb_ternary, sym, sym_force  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
G = dict(G11=-0.31, G12=0.92, G13=0.73, G22=-0.27, G23=1.04, G33=-0.18)
VISC, TAU_PHI, TAU_THETA = 0.09, 0.87, 1.21


def _evalf(expr, values):
    if not isinstance(expr, sympy.Basic):
        return sympy.Float(expr, 30)
    subs = {}
    for s in expr.free_symbols:
        if s not in values:
            raise KeyError('unbound symbol %s' % s)
        subs[s] = sympy.Float(values[s], 30)
    return expr.subs(subs).evalf(30)


def make_sim(grid):
    cfg = types.SimpleNamespace(grid=grid.__name__, visc=VISC, tau_phi=TAU_PHI, tau_theta=TAU_THETA, incompressible=False,
                                minimize_roundoff=False, sc_potential='linear', force_implementation='guo', **G)
    return lb_ternary.LBTernaryFluidShanChen(cfg), cfg


def capture(grid, rng):
    sim, cfg = make_sim(grid)
    S = sim.S
    consts = sim.constants()
    names = sorted(k for k in consts if k.startswith('G'))
    out = dict(coupling_names=np.array(names), coupling_values=np.array([float(consts[k]) for k in names]),
               force_couplings=np.array([list(k) for k in sim._force_couplings.keys()]),
               force_coupling_names=np.array(list(sim._force_couplings.values())),
               G=np.array([G[k] for k in ('G11', 'G12', 'G13', 'G22', 'G23', 'G33')]),
               tau=np.array([sym.relaxation_time(VISC), TAU_PHI, TAU_THETA]))
    n, dim = 32, grid.dim
    dens = rng.uniform(0.3, 1.5, (n, 3))
    v = rng.uniform(-1.0, 1.0, (n, dim))
    v = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.0, 0.1, n)[:, None]
    v[0] = 0.0
    accel = rng.uniform(-0.05, 0.05, (n, 3, dim))
    eqs = [eq(grid, cfg) for eq in sim.equilibria]
    dens_syms = [S.rho, S.phi, S.theta]
    taus = out['tau']
    feq, guo = [], []
    for k in range(n):
        values = {S.rho: dens[k, 0], S.phi: dens[k, 1], S.theta: dens[k, 2]}
        for d in range(dim):
            values[grid.v[d]] = v[k, d]
        row_f, row_g = [], []
        for num in range(3):
            eq = eqs[num]
            vals = dict(values)
            for lv in eq.local_vars:
                vals[lv.lhs] = _evalf(lv.rhs, vals)
            row_f.append([float(_evalf(e, vals)) for e in eq.expression])
            pref = sym_force.guo_external_force_pref(grid, cfg, grid_num=num)
            gv = dict(values)
            gv[S.relaxation_times[num]] = taus[num]
            gv[S.densities[num]] = dens[k, num]
            ea = sym_force.accel_vector(grid, num)
            for d in range(dim):
                gv[ea[d]] = accel[k, num, d]
            pref_val = _evalf(pref, gv)
            gv[sympy.Symbol('pref')] = pref_val
            row_g.append([float(_evalf(e, gv)) for e in sym_force.guo_external_force(grid, grid_num=num)])
        feq.append(row_f)
        guo.append(row_g)
    out.update(dens=dens, v=v, accel=accel, feq=np.array(feq), guo=np.array(guo))
    x = sympy.Symbol('x')
    psi_rho = np.concatenate([[0.0, 1.0], rng.uniform(0.01, 3.0, 30)])
    out['psi_rho'] = psi_rho
    for name, fn in sym.SHAN_CHEN_POTENTIALS.items():
        expr = fn('x')          # the potentials take the name of the field
        out['psi_' + name] = np.array([float(_evalf(expr, {x: r})) for r in psi_rho])
    return out


if __name__ == '__main__':
    for grid in (sym.D2Q9, sym.D3Q19):
        rng = np.random.RandomState(33000 + grid.Q)
        data = capture(grid, rng)
        path = os.path.join(OUT, 'arith_sc3_%s.npz' % grid.__name__)
        np.savez(path, **data)
        print(path, {k: np.shape(v) for k, v in data.items()})
