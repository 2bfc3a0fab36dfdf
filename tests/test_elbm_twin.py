"""The numpy twin of the entropic collision (tests/_elbm_twin.py) against values of the reference's own sympy objects
(tests/golden/arith_elbm_*.npz, tools/capture_elbm.py), and the properties the GPU tests rely on: the twin is what the
HIP kernels of --model=elbm are compared with."""
import os

import numpy as np
import pytest

from sailfish_amd import sym
from tests import _elbm_twin as tw

GRIDS = {'D2Q9': sym.D2Q9, 'D3Q19': sym.D3Q19}
EPS = np.finfo(np.float64).eps
# the shear layer of tests/test_gpu_elbm.py: Re = U n / visc = 10^4 on 64 nodes, a layer two nodes thick
SHEAR = dict(n=64, U=0.05, k=80.0, delta=0.05, visc=3e-4, steps=800)


def shear_layer(n, U, k, delta, **_):
    """Doubly periodic shear layer (Minion & Brown): u_x = U tanh(k (y - 1/4)) resp. U tanh(k (3/4 - y)),
    u_y = delta U sin(2 pi (x + 1/4))."""
    y, x = np.meshgrid((np.arange(n) + 0.5) / n, (np.arange(n) + 0.5) / n, indexing='ij')
    ux = np.where(y <= 0.5, U * np.tanh(k * (y - 0.25)), U * np.tanh(k * (0.75 - y)))
    uy = delta * U * np.sin(2 * np.pi * (x + 0.25))
    return np.ones((n, n)), [ux, uy]


def kinetic_energy(rho, v):
    return float((np.asarray(rho, dtype=np.float64) * sum(np.asarray(c, dtype=np.float64) ** 2 for c in v)).sum())


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, 'arith_elbm_%s.npz' % name))


def _v3(grid, v):
    return [v[:, d] for d in range(grid.dim)] + [np.zeros(v.shape[0])] * (3 - grid.dim)


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_weights_equilibria_and_series_reproduce_the_reference(golden_dir, name):
    grid, G = GRIDS[name], _golden(golden_dir, name)
    assert np.array_equal(np.array([float(w) for w in grid.entropic_weights]), G['entropic_weights'])
    rho, v = G['rho'], _v3(grid, G['v'])
    assert np.max(np.linalg.norm(G['v'], axis=1)) > 0.14
    for mine, key in ((tw.feq_bgk(grid, rho, v), 'feq_bgk'), (tw.feq_entropic(grid, rho, v), 'feq_entropic')):
        err = np.max(np.abs(mine.T - G[key]) / G[key])
        assert err < 16 * EPS, (key, err)           # a product of up to 10 factors, each rounded once
    a = G['series_a']
    alpha = tw.alpha_series(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    assert np.max(np.abs(alpha - G['series_alpha'])) < 16 * EPS
    assert np.ptp(G['series_alpha']) > 1e-4         # the fixture exercises the series, not just its leading 2


def test_product_form_moments():
    """D2Q9: rho and rho v to rounding (the product form is exact there).  D3Q19 at order 8: rho exactly at rest, and along
    the axes up to |v| = 0.15 what the reference's tests/sym_equilibrium.py asserts: |rho' / rho - 1| < 1e-7 and the
    momentum to 7 places."""
    rng = np.random.RandomState(3)
    rho = rng.uniform(0.9, 1.1, 64)
    v = rng.uniform(-0.1, 0.1, (64, 2))
    fe = tw.feq_entropic(sym.D2Q9, rho, _v3(sym.D2Q9, v))
    e = np.array(sym.D2Q9.basis)
    assert np.max(np.abs(fe.sum(0) - rho)) < 8 * EPS
    assert np.max(np.abs(e.T.dot(fe) - (rho * v.T))) < 8 * EPS
    g = sym.D3Q19
    e = np.array(g.basis)
    one = np.ones(1)
    assert tw.feq_entropic(g, 1.3 * one, [0 * one] * 3).sum() == pytest.approx(1.3, abs=2 * EPS)
    for c in (0.0, 0.05, 0.1, 0.15, -0.05, -0.1, -0.15):
        for axis in range(3):
            v = [c * one if d == axis else 0 * one for d in range(3)]
            fe = tw.feq_entropic(g, one, v)[:, 0]
            assert abs(fe.sum() - 1.0) < 1e-7
            assert abs(e[:, axis].dot(fe) - c) < 5e-8


@pytest.mark.parametrize('name', sorted(GRIDS))
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_regimes_of_the_fixture_states(golden_dir, name, dtype):
    grid, G = GRIDS[name], _golden(golden_dir, name)
    for key, ent in (('bgk', False), ('entropic', True)):
        dev, regime = G['dev_' + key], G['regime_' + key]
        assert all((regime == r).sum() >= 8 for r in (0, 1, 2))
        for thr in (1e-6, 0.01):
            assert not np.any((dev > thr / 1.25) & (dev < thr * 1.25))
        r = tw.collide(grid, G['f_' + key].T.astype(dtype), 0.01, entropic_eq=ent)
        assert np.array_equal(r['regime'], regime)
        if dtype is np.float64:
            assert np.max(np.abs(r['dev'] - dev) / dev) < 1e-6        # cancellation in feq - f at dev = 1e-9
        assert r['ok'].all()


@pytest.mark.parametrize('name', sorted(GRIDS))
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_small_deviation_is_bgk(golden_dir, name, dtype):
    """dev < 1e-6: alpha = 2, and 2 beta = 1 / tau: the BGK relaxation at the same viscosity, to rounding."""
    grid, G = GRIDS[name], _golden(golden_dir, name)
    f = G['f_bgk'][G['regime_bgk'] == 0].T.astype(dtype)
    R = f.dtype.type
    for visc in (0.1, 0.003):
        r = tw.collide(grid, f, visc)
        assert np.all(r['alpha'] == 2)
        omega = R(1.0 / sym.relaxation_time(visc))
        bgk = f + omega * r['fneq']
        assert np.max(np.abs(r['f'] - bgk) / bgk) < 4 * np.finfo(dtype).eps


@pytest.mark.parametrize('name', sorted(GRIDS))
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('log2', [False, True])
def test_newton_meets_its_stop_rule(golden_dir, name, dtype, log2):
    """Every Newton-regime state, cold (from 2) and warm (from its own answer): the result is inside [1, max_alpha] and
    either |H(f + alpha fneq) - H(f)| is below the tolerance or the last step of alpha was (both in the twin's own
    arithmetic: that is the rule)."""
    grid, G = GRIDS[name], _golden(golden_dir, name)
    tol = tw.default_entropy_tolerance(dtype)
    for key, ent in (('bgk', False), ('entropic', True)):
        f = G['f_' + key][G['regime_' + key] == 2].T.astype(dtype)
        cold = tw.collide(grid, f, 0.01, entropic_eq=ent, log2=log2)
        warm = tw.collide(grid, f, 0.01, entropic_eq=ent, log2=log2, alpha_start=cold['alpha'])
        for r in (cold, warm):
            assert r['ok'].all()
            alpha, fneq = r['alpha'], r['fneq']
            assert np.all(alpha >= 1) and np.all(alpha <= tw.max_alpha(f, fneq))
            dh = tw.entropy(grid, f + alpha * fneq, log2) - tw.entropy(grid, f, log2)
            stalled = ~(np.abs(dh) < f.dtype.type(tol))
            if stalled.any():           # ended by the alpha rule: one more step moves alpha by less than alpha_tolerance
                again, ok, steps = tw.newton(grid, f[:, stalled], fneq[:, stalled], alpha[stalled], tol, 1e-10, log2)
                assert ok.all() and np.all(steps == 0) and np.array_equal(again, alpha[stalled])
        assert np.max(np.abs(warm['alpha'] - cold['alpha'])) < 1e-3
        assert np.ptp(cold['alpha']) > 1e-3


def test_give_up_path():
    """What the reference answers with die(): the twin (and the kernel, which sets the module's invalid-value word)
    reports the node, leaves its populations alone and keeps every other node's result."""
    grid = sym.D2Q9
    w = np.array([float(x) for x in grid.weights])
    f = np.array([w, w * (1 + 0.3 * np.cos(np.arange(9))), w]).T.copy()
    f[3, 2] = -0.05                                   # a negative population: the entropy is not a number
    r = tw.collide(grid, f, 0.01)
    assert list(r['ok']) == [True, True, False]
    assert np.array_equal(r['f'][:, 2], f[:, 2]) and r['regime'][2] == 2
    assert r['regime'][1] == 2 and 1 <= r['alpha'][1] and not np.array_equal(r['f'][:, 1], f[:, 1])
    # more than 1000 steps: tolerances nothing can meet
    alpha, ok, steps = tw.newton(grid, f[:, 1:2], r['fneq'][:, 1:2], np.array([2.0]), 0.0, 0.0)
    assert not ok[0] and steps[0] == 1001


def test_shear_layer_survives_in_the_twin():
    """The parameters of the GPU test (tests/test_gpu_elbm.py: D2Q9, 64 x 64, single precision): the reference algorithm
    itself gets through -- no node gives up, everything stays finite, the kinetic energy never exceeds its initial value
    and the Newton branch is really taken."""
    rho, v = shear_layer(**SHEAR)
    t = tw.ElbmTwin.from_fields(sym.D2Q9, rho, v, SHEAR['visc'], dtype=np.float32)
    k0 = kinetic_energy(*t.macros())
    for _ in range(SHEAR['steps'] // 100):
        t.run(100)
        assert np.isfinite(t.f).all() and t.failed == 0
        assert kinetic_energy(*t.macros()) <= k0
    assert t.regime_counts[2] > 0.2 * t.regime_counts.sum()
    assert t.alpha.min() >= 1 and np.ptp(t.alpha) > 1e-3


def test_streaming_and_bounce_back():
    """The twin's box: mass is conserved to rounding in a closed box of full-way bounce-back walls, and a uniform
    periodic box is invariant under streaming."""
    grid, n = sym.D2Q9, 12
    wall = np.zeros((n, n), dtype=bool)
    wall[0] = wall[-1] = wall[:, 0] = wall[:, -1] = True
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    v = [0.03 * np.sin(2 * np.pi * y / n), 0.02 * np.cos(2 * np.pi * x / n)]
    t = tw.ElbmTwin.from_fields(grid, np.ones((n, n)), v, 0.01, wall=wall)
    m0 = t.f.sum()
    t.run(30)
    assert abs(t.f.sum() - m0) < 1e-12 * m0
    u = tw.ElbmTwin.from_fields(grid, 1.02 * np.ones((n, n)), [0.04 * np.ones((n, n)), -0.01 * np.ones((n, n))], 0.01)
    f0 = u.f.copy()
    u.run(3)
    assert np.max(np.abs(u.f - f0)) < 1e-15
