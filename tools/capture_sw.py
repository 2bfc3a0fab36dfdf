#!/usr/bin/env python3
"""Generate tests/golden/arith_sw_D2Q9.npz from the reference's sympy objects of the shallow-water model
(sym_equilibrium.shallow_water_equilibrium, the equilibrium of lb_single.LBFreeSurface).

Runs only where the reference is importable (tools/ref_shim.py); the fixture is data -- inputs and expected values -- and
nothing in tests/ or the product reads the reference at run time.  Every expected value is the reference's own expression
object evaluated at 30 digits and rounded to float64.

    PYTHONPATH=tools python tools/capture_sw.py

    gravity     [2]            0.001 (the default of --gravity) and 0.05
    h           [n]            water depths in [0.5, 1.5], n = 48
    v           [n, 2]         velocities, |v| <= 0.1; v[0] = 0
    feq         [2, n, 9]      the nine expressions, per gravity and state.  Rows 1..8 are what the kernels compute; row 0 is
                               the reference's rest population, which exceeds the conserving one by 2 h v^2
                               (tests/golden/README_sw.md)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: F401  (installs import stubs, puts the reference on sys.path)

import numpy as np
import sympy

from sailfish import sym, sym_equilibrium  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
GRAVITY = (0.001, 0.05)


def _evalf(expr, values):
    if not isinstance(expr, sympy.Basic):
        return sympy.Float(expr, 30)
    subs = {}
    for s in expr.free_symbols:
        if s not in values:
            raise KeyError('unbound symbol %s' % s)
        subs[s] = sympy.Float(values[s], 30)
    return expr.subs(subs).evalf(30)


def capture(rng):
    grid, S = sym.D2Q9, sym.S
    eq = sym_equilibrium.shallow_water_equilibrium(grid, None)
    assert not eq.local_vars and len(eq.expression) == 9
    n = 48
    h = rng.uniform(0.5, 1.5, n)
    v = rng.uniform(-1.0, 1.0, (n, 2))
    v = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.0, 0.1, n)[:, None]
    v[0] = 0.0
    feq = np.zeros((len(GRAVITY), n, 9))
    for a, g in enumerate(GRAVITY):
        for k in range(n):
            values = {S.rho: h[k], S.gravity: g, grid.v[0]: v[k, 0], grid.v[1]: v[k, 1]}
            feq[a, k] = [float(_evalf(e, values)) for e in eq.expression]
    return dict(gravity=np.array(GRAVITY), h=h, v=v, feq=feq)


if __name__ == '__main__':
    data = capture(np.random.RandomState(31909))
    path = os.path.join(OUT, 'arith_sw_D2Q9.npz')
    np.savez(path, **data)
    print(path, {k: np.shape(x) for k, x in data.items()})
