#!/usr/bin/env python3
"""Generate tests/golden/arith_tms_{D2Q9,D3Q19}.npz: what a Tamm-Mott-Smith wall node (NTWallTMS) computes, from the
reference's own sympy objects (sym.ex_rho, sym.ex_velocity, sym_equilibrium.bgk_equilibrium, sym_force.guo_external_force
and guo_external_force_pref), composed in the order of the templates (boundary.mako:631-648, 696-723;
lb_single_fluid.mako:185-228; relaxation_common.mako:110-149).

Runs only where the reference is importable (tools/ref_shim.py); the fixtures are data -- inputs and expected values --
and nothing in tests/ or the product reads the reference at run time.  Every value is evaluated at 30 digits, carried at
30 digits from one step to the next, and rounded to float64 at the end.

    PYTHONPATH=tools python tools/capture_tms.py

Per lattice:
    f                  [n, Q]        seeded non-equilibrium populations: rho in [0.9, 1.1], |u| <= 0.1, each population of
                                     the equilibrium scaled by 1 + 0.05 xi
    accel              [n, dim]      body-force accelerations of the forced variants
    visc               [1]
    words, use_tags    [m], [m]      the node's orientation word: an orientation code (use_tags 0; every orientation) or a
                                     link-tag word (use_tags 1; bit i - 1 set = direction i points to a wet node): the
                                     plane walls, and the edge and corner nodes of a duct
    missing            [m, Q]        1 = direction i points to a non-fluid node (population opp(i) is unknown)
and for every variant <form>_<force>, form in compressible / incompressible / roundoff, force in none / guo
(the roundoff variants work on f_i - w_i and their density is rho - 1):
    <v>_tg_rho, <v>_tg_v          [m, n], [m, n, dim]   the target state: moments of the populations as loaded
    <v>_repaired                  [m, n, Q]             unknown populations replaced by feq_i(tg_rho, tg_v)
    <v>_rho, <v>_v                [m, n], [m, n, dim]   instantaneous density and velocity of the repaired populations
    <v>_v_out                     [m, n, dim]           the velocity after the relaxation (v + a / 2 under a force)
    <v>_post                      [m, n, Q]             BGK-relaxed, plus feq(tg_rho, tg_v), minus feq(rho, v_out): what the
                                                        half-way bounce-back store and the propagation then move
"""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: F401  (installs import stubs, puts the reference on sys.path)

import numpy as np
import sympy

from sailfish import sym, sym_equilibrium, sym_force  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
VISC = 0.02
DIGITS = 30


class _Cfg(object):
    def __init__(self, incompressible=False, minimize_roundoff=False):
        self.incompressible = incompressible
        self.minimize_roundoff = minimize_roundoff


def _F(x):
    return x if isinstance(x, sympy.Basic) else sympy.Float(x, DIGITS)


def _evalf(expr, subs):
    """expr with its symbols replaced by name, at DIGITS digits (a sympy Float)."""
    if not isinstance(expr, sympy.Basic):
        return _F(float(expr))
    m = {}
    for s in expr.free_symbols:
        if s.name not in subs:
            raise KeyError('unbound symbol %s in %s' % (s.name, expr))
        m[s] = _F(subs[s.name])
    return expr.subs(m).evalf(DIGITS)


def _fi_subs(grid, f):
    return {'fi->%s' % n: v for n, v in zip(grid.idx_name, f)}


def _macro_subs(grid, rho, v, inc):
    d = {'g0m0': rho, 'rho': rho, 'rho0': _F(1.0) if inc else rho}
    for c, val in zip('xyz', v):
        d['g0m1' + c] = val
    return d


def node_words(grid):
    """(word, use_tags, missing[Q]) of every orientation code, and of the link-tag words of nodes on one, two and (3-D)
    three walls of a duct: direction i is missing iff it has a component pointing out through one of the node's walls."""
    e = np.array([[int(c) for c in b] for b in grid.basis], dtype=np.int64)
    rows = []
    for o in range(1, 2 * grid.dim + 1):
        miss = np.zeros(grid.Q, dtype=np.int64)
        for i in sym.get_missing_dists(grid, o):          # unknown populations: their opposites point to the wall
            miss[grid.idx_opposite[i]] = 1
        rows.append((o, 0, miss))
    for normals in itertools.product((-1, 0, 1), repeat=grid.dim):     # inward normal component per axis, 0: no wall
        if not any(normals):
            continue
        miss = np.zeros(grid.Q, dtype=np.int64)
        for i in range(1, grid.Q):
            if any(n != 0 and e[i, ax] * n < 0 for ax, n in enumerate(normals)):
                miss[i] = 1
        word = sum((1 - int(miss[i])) << (i - 1) for i in range(1, grid.Q))
        rows.append((word, 1, miss))
    return rows


def capture(grid, rng, n=5):
    dim, Q = grid.dim, grid.Q
    opp = grid.idx_opposite
    wts = np.array([float(w) for w in grid.weights])
    rho = rng.uniform(0.9, 1.1, n)
    v = rng.uniform(-1.0, 1.0, (n, dim))
    v = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.02, 0.1, n)[:, None]
    eq_std = sym_equilibrium.bgk_equilibrium(grid, _Cfg()).expression
    f = np.zeros((n, Q))
    for k in range(n):
        subs = _macro_subs(grid, _F(rho[k]), [_F(x) for x in v[k]], False)
        f[k] = [float(_evalf(e, subs)) for e in eq_std]
    f = f * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (n, Q)))
    accel = rng.uniform(-1e-4, 1e-4, (n, dim))
    words = node_words(grid)
    m = len(words)
    out = {'f': f, 'accel': accel, 'visc': np.array([VISC]),
           'words': np.array([w[0] for w in words], dtype=np.int64),
           'use_tags': np.array([w[1] for w in words], dtype=np.int64),
           'missing': np.array([w[2] for w in words], dtype=np.int64)}
    tau = _F(sym.relaxation_time(VISC))
    guo = sym_force.guo_external_force(grid, grid_num=0)
    for form in ('compressible', 'incompressible', 'roundoff'):
        inc, ro = form == 'incompressible', form == 'roundoff'
        cfg = _Cfg(incompressible=inc, minimize_roundoff=ro)
        eq = sym_equilibrium.bgk_equilibrium(grid, cfg).expression
        ex_rho = sym.ex_rho(grid, 'fi', inc, minimize_roundoff=ro)
        ex_v = [sym.ex_velocity(grid, 'fi', d, cfg) for d in range(dim)]
        pref_e = sym_force.guo_external_force_pref(grid, cfg, grid_num=0)

        def macro(fi):
            subs = _fi_subs(grid, fi)
            r = _evalf(ex_rho, subs)
            subs.update({'g0m0': r, 'rho': r, 'rho0': _F(1.0) if inc else r})
            return r, [_evalf(e, subs) for e in ex_v]

        for force in ('none', 'guo'):
            key = '%s_%s' % (form, force)
            res = {k: np.zeros((m, n) + s) for k, s in (('tg_rho', ()), ('tg_v', (dim,)), ('repaired', (Q,)), ('rho', ()),
                                                        ('v', (dim,)), ('v_out', (dim,)), ('post', (Q,)))}
            for w, (_, _, miss) in enumerate(words):
                for k in range(n):
                    fi = [_F(x) for x in (f[k] - wts if ro else f[k])]
                    # fixMissingDistributions (boundary.mako:631-648)
                    tg_rho, tg_v = macro(fi)
                    tsubs = _macro_subs(grid, tg_rho, tg_v, inc)
                    fe_tg = [_evalf(e, tsubs) for e in eq]
                    for i in range(1, Q):
                        if miss[i]:
                            fi[opp[i]] = fe_tg[opp[i]]
                    # getMacro
                    r, vv = macro(fi)
                    # relaxation (relaxation_common.mako:110-149, relaxation.mako:127-132)
                    a = [_F(x) for x in accel[k]] if force == 'guo' else None
                    v_out = [x + a[d] / 2 for d, x in enumerate(vv)] if a else list(vv)
                    subs = _macro_subs(grid, r, v_out, inc)
                    fe = [_evalf(e, subs) for e in eq]
                    post = [fi[i] + (fe[i] - fi[i]) / tau for i in range(Q)]
                    if a:
                        subs.update({'g0ea' + c: a[j] for j, c in enumerate('xyz'[:dim])})
                        subs['tau0'] = tau
                        subs['pref'] = _evalf(pref_e, subs)
                        post = [post[i] + _evalf(guo[i], subs) for i in range(Q)]
                    # postcollisionBoundaryConditions (boundary.mako:696-719): + feq(target), - feq(rho, v)
                    post = [post[i] + fe_tg[i] - fe[i] for i in range(Q)]
                    res['tg_rho'][w, k], res['tg_v'][w, k] = float(tg_rho), [float(x) for x in tg_v]
                    res['repaired'][w, k] = [float(x) for x in fi]
                    res['rho'][w, k], res['v'][w, k] = float(r), [float(x) for x in vv]
                    res['v_out'][w, k] = [float(x) for x in v_out]
                    res['post'][w, k] = [float(x) for x in post]
            for k2, arr in res.items():
                out['%s_%s' % (key, k2)] = arr
    return out


if __name__ == '__main__':
    for grid in (sym.D2Q9, sym.D3Q19):
        rng = np.random.RandomState(20250 + grid.Q)
        data = capture(grid, rng)
        path = os.path.join(OUT, 'arith_tms_%s.npz' % grid.__name__)
        np.savez(path, **data)
        print(path, {k: v.shape for k, v in data.items()})
