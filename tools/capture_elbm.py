#!/usr/bin/env python3
"""Generate tests/golden/arith_elbm_{D2Q9,D3Q19}.npz from the reference's sympy objects of the entropic model
(sym.entropic_weights, sym_equilibrium.bgk_equilibrium / elbm_equilibrium / elbm_d3q19_equilibrium, sym.alpha_series).

Runs only where the reference is importable (tools/ref_shim.py); the fixtures are data -- inputs and expected values --
and nothing in tests/ or the product reads the reference at run time.  Every expected value is the reference's own
expression object evaluated at 30 digits and rounded to float64.

    PYTHONPATH=tools python tools/capture_elbm.py

Per lattice:
    entropic_weights                      [Q]
    rho, v                                [n], [n, dim]      macroscopic states, |v| up to 0.15
    feq_bgk, feq_entropic                 [n, Q]             the two equilibria on them
    series_a, series_alpha                [m, 4], [m]        a1..a4 (with the factors of ComputeACoeff) and alpha_series()
    f_bgk, dev_bgk, regime_bgk            [k, Q], [k], [k]   population states around the polynomial equilibrium, their
    f_entropic, dev_entropic, regime_...                     dev = max |feq / f - 1| and regime (0: < 1e-6, 1: < 0.01,
                                                             2: Newton); the same around the product form
No state has dev within a factor 1.25 of 1e-6 or 0.01.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: F401  (installs import stubs, puts the reference on sys.path)

import numpy as np
import sympy

from sailfish import sym, sym_equilibrium  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')


class _Cfg(object):
    incompressible = False
    minimize_roundoff = False
    entropic_equilibrium = False


def _evalf(expr, subs):
    if isinstance(expr, (int, float)):
        return float(expr)
    m = {}
    for s in expr.free_symbols:
        if s.name not in subs:
            raise KeyError('unbound symbol %s' % s.name)
        m[s] = sympy.Float(subs[s.name], 30) if not isinstance(subs[s.name], sympy.Basic) else subs[s.name]
    return expr.subs(m).evalf(30)


def _macro_subs(grid, rho, v):
    d = {str(sym.S.rho): float(rho), 'rho0': float(rho)}
    for s, val in zip(grid.v, v):
        d[str(s)] = float(val)
    return d


def equilibrium(grid, eq, rho, v):
    """The populations of EqDef `eq` at (rho, v): local variables first, in order, as the kernel would."""
    subs = _macro_subs(grid, rho, v)
    for lv in eq.local_vars:
        subs[str(lv.lhs)] = _evalf(lv.rhs, subs)
    return np.array([float(_evalf(e, subs)) for e in eq.expression])


def moments(grid, f):
    rho = float(np.sum(f))
    v = [float(sum(float(e[d]) * fi for e, fi in zip(grid.basis, f)) / rho) for d in range(grid.dim)]
    return rho, v


def deviation(grid, eq, f):
    rho, v = moments(grid, f)
    fe = equilibrium(grid, eq, rho, v)
    return float(np.max(np.abs((fe - f) / f))), fe


def a_coeffs(f, fneq):
    """ComputeACoeff (entropic.mako:9-35) in float64."""
    a = np.zeros(4)
    for fi, t in zip(f, fneq):
        inv = 1.0 / fi
        p = t * t * inv
        t = t * inv
        for k in range(4):
            a[k] += p
            p = p * t
    return a * np.array([0.5, -1.0 / 6.0, 1.0 / 12.0, -1.0 / 20.0])


def states(grid, eq, rng, targets):
    """Populations eq(rho, v) (1 + A xi) with the amplitude A tuned so that dev lands near each target."""
    fs, devs = [], []
    for tgt in targets:
        rho = rng.uniform(0.95, 1.05)
        v = rng.uniform(-0.08, 0.08, grid.dim)
        base = equilibrium(grid, eq, rho, v)
        xi = rng.uniform(-1.0, 1.0, grid.Q)
        amp = tgt
        for _ in range(6):
            f = base * (1.0 + amp * xi)
            dev, _ = deviation(grid, eq, f)
            if 0.8 < dev / tgt < 1.25:
                break
            amp *= tgt / dev
        for thr in (1e-6, 0.01):
            assert not (thr / 1.25 <= dev <= thr * 1.25), dev
        assert np.all(f > 0)
        fs.append(f)
        devs.append(dev)
    devs = np.array(devs)
    return np.array(fs), devs, np.where(devs < 1e-6, 0, np.where(devs < 0.01, 1, 2))


def capture(grid, rng):
    out = {'entropic_weights': np.array([float(w) for w in grid.entropic_weights])}
    eq_bgk = sym_equilibrium.bgk_equilibrium(grid, _Cfg())
    eq_ent = sym_equilibrium.elbm_d3q19_equilibrium(grid) if grid is sym.D3Q19 else sym_equilibrium.elbm_equilibrium(grid)
    n = 40
    rho = rng.uniform(0.9, 1.1, n)
    v = rng.uniform(-1.0, 1.0, (n, grid.dim))
    v = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.0, 0.15, n)[:, None]
    v[0] = 0.0
    v[1] = np.array([0.15] + [0.0] * (grid.dim - 1))
    out['rho'], out['v'] = rho, v
    out['feq_bgk'] = np.array([equilibrium(grid, eq_bgk, r, u) for r, u in zip(rho, v)])
    out['feq_entropic'] = np.array([equilibrium(grid, eq_ent, r, u) for r, u in zip(rho, v)])
    targets = np.concatenate([10.0 ** rng.uniform(-8.5, -6.8, 10), 10.0 ** rng.uniform(-5.6, -2.3, 14),
                              10.0 ** rng.uniform(-1.7, -0.25, 14)])
    series = sym.alpha_series()
    sa, sv = [], []
    for name, eq in (('bgk', eq_bgk), ('entropic', eq_ent)):
        f, dev, regime = states(grid, eq, rng, targets)
        assert all((regime == r).sum() >= 8 for r in (0, 1, 2)), regime
        out['f_' + name], out['dev_' + name], out['regime_' + name] = f, dev, regime
        for fk in f[regime == 1]:
            _, fe = deviation(grid, eq, fk)
            a = a_coeffs(fk, fe - fk)
            sa.append(a)
            sv.append(float(_evalf(series, {'a%d' % (i + 1): a[i] for i in range(4)})))
    out['series_a'], out['series_alpha'] = np.array(sa), np.array(sv)
    return out


if __name__ == '__main__':
    for grid in (sym.D2Q9, sym.D3Q19):
        rng = np.random.RandomState(20240 + grid.Q)
        data = capture(grid, rng)
        path = os.path.join(OUT, 'arith_elbm_%s.npz' % grid.__name__)
        np.savez(path, **data)
        print(path, {k: v.shape for k, v in data.items()})
