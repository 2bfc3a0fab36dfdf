"""The numpy twin of the free-energy binary fluid (tests/_fe_twin.py) against values of the reference's own sympy objects
(tests/golden/arith_fe_*.npz, tools/capture_fe.py), and the properties the GPU tests rely on: the twin is what the HIP
kernels of LBBinaryFluidFreeEnergy are compared with."""
import os

import numpy as np
import pytest

from sailfish_amd import sym
from tests import _fe_twin as tw

GRIDS = {'D2Q9': sym.D2Q9, 'D3Q19': sym.D3Q19}
EPS = float(np.finfo(np.float64).eps)
TABLES = ('wi', 'wxx', 'wyy', 'wzz', 'wxy', 'wyz', 'wxz')
# the flat-interface box of test_flat_interfaces_stay_tanh_profiles (and of profiles/NOTES.md)
FLAT = dict(shape=(8, 64), kappa=0.04, A=0.04, tau_a=1.0, tau_b=1.0, tau_phi=1.0, Gamma=0.5, steps=2000)


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, 'arith_fe_%s.npz' % name))


def _params(G):
    return dict((k, float(G[k])) for k in ('A', 'kappa', 'Gamma', 'tau_a', 'tau_b'))


def _cols(a):
    return [a[:, d] for d in range(a.shape[1])]


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_weight_tables_equilibria_and_relaxation_time_reproduce_the_reference(golden_dir, name):
    """Bounds from the operation count.  A population i >= 1 is wi (bulk + rho h) + kappa q: pb 6 operations, bulk 3,
    |v|^2 / 2 up to 6, h 4, the bracket and the product with wi 3, q up to 8, the last product and sum 2 -- 32 roundings of
    half an ulp of intermediates below 1.25 (rho <= 1.2), i.e. 20 eps, and half an ulp of the fixture's own rounding: 24
    eps.  The rest population is rho minus the sum of the Q - 1 others: their errors, scaled by the largest wi that
    multiplies the bracket, plus one rounding of a partial sum below rho each.  The order-parameter populations are formed
    from fewer operations of smaller values: the same bounds hold.  tau0 is three roundings of values below 2."""
    grid, G = GRIDS[name], _golden(golden_dir, name)
    p = _params(G)
    w = tw.weight_tables(grid)
    for t in TABLES:
        assert np.array_equal(np.array(w[t]), G[t]), t
    assert (G['phi'] < -1).sum() >= 3 and (G['phi'] > 1).sum() >= 3 and np.max(np.linalg.norm(G['v'], axis=1)) > 0.09
    assert np.all(G['grad'][:24] == 0) and np.all(np.abs(G['grad'][24:]).max(axis=1) > 0)
    rho, phi, lap, v, grad = G['rho'], G['phi'], G['lap'], _cols(G['v']), _cols(G['grad'])
    ff = tw.feq_fluid(grid, rho, phi, lap, v, grad, p['A'], p['kappa'], np.float64)
    fo = tw.feq_order(grid, phi, lap, v, p['A'], p['kappa'], p['Gamma'], np.float64)
    rest = (grid.Q - 1) * (24 * max(w['wi']) + 0.6) * EPS
    for mine, key in ((ff, 'feq_fluid'), (fo, 'feq_order')):
        err = np.abs(mine.T - G[key])
        print('%s %s: rest %.2e (bound %.2e), others %.2e (bound %.2e)' % (name, key, err[:, 0].max(), rest,
                                                                           err[:, 1:].max(), 24 * EPS))
        assert err[:, 1:].max() <= 24 * EPS, key
        assert err[:, 0].max() <= rest, key
    assert np.max(np.abs(tw.tau0(phi, p['tau_a'], p['tau_b'], np.float64) - G['tau0'])) <= 3 * EPS
    assert np.all(tw.tau0(phi[phi < -1], p['tau_a'], p['tau_b'], np.float64) == p['tau_b'])
    assert np.all(tw.tau0(phi[phi > 1], p['tau_a'], p['tau_b'], np.float64) == p['tau_a'])


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_equilibria_carry_rho_and_phi(golden_dir, name):
    """The rest population is rho (phi) minus the sum of the others; summing all Q again, in another order, differs by at
    most one rounding of a partial sum below |rho| (1.3 for phi) per term."""
    grid, G = GRIDS[name], _golden(golden_dir, name)
    p = _params(G)
    rho, phi, lap, v, grad = G['rho'], G['phi'], G['lap'], _cols(G['v']), _cols(G['grad'])
    ff = tw.feq_fluid(grid, rho, phi, lap, v, grad, p['A'], p['kappa'], np.float64)
    fo = tw.feq_order(grid, phi, lap, v, p['A'], p['kappa'], p['Gamma'], np.float64)
    assert np.max(np.abs(tw.density(ff) - rho)) <= grid.Q * 0.5 * EPS * 1.3
    assert np.max(np.abs(tw.density(fo) - phi)) <= grid.Q * 0.5 * EPS * 1.3
    # and the first moment of the fluid's equilibrium is rho v (|rho v| <= 0.12: Q products and sums of such values)
    for d in range(grid.dim):
        assert np.max(np.abs(tw.momentum(grid, ff, d) - rho * v[d])) <= 2 * grid.Q * EPS * 0.25


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_stencils_are_exact_on_linear_and_quadratic_fields(name):
    """Pooley & Furtado's stencils: the gradient of a linear field and the Laplacian of a quadratic one, to the rounding of
    the divisions by 12, 6 and 3 (small integer data: every sum is exact)."""
    grid = GRIDS[name]
    b = tw.basis(grid)
    a = [3.0, -2.0, 5.0][:grid.dim]
    lin = lambda x: 7.0 + sum(ac * xc for ac, xc in zip(a, x))              # noqa: E731
    x0 = [4, -3, 2][:grid.dim]
    lap, grad = tw.stencil(grid, lambda i: np.float64(lin([p + e for p, e in zip(x0, b[i])])), np.float64(lin(x0)), np.float64)
    assert all(abs(g - ac) <= 4 * EPS * abs(ac) for g, ac in zip(grad, a))
    assert abs(lap) <= 64 * EPS              # cancels sums of magnitude up to 4 |field| ~ 200 after divisions
    if grid.dim == 3:
        quad = lambda x: 2.0 * x[0] ** 2 + 3.0 * x[1] ** 2 - x[2] ** 2 + x[0] * x[1] - 2.0 * x[1] * x[2] + lin(x)   # noqa: E731
        want = 2 * 2.0 + 2 * 3.0 - 2 * 1.0
    else:
        quad = lambda x: 2.0 * x[0] ** 2 + 3.0 * x[1] ** 2 + x[0] * x[1] + lin(x)   # noqa: E731
        want = 2 * 2.0 + 2 * 3.0
    lap, grad = tw.stencil(grid, lambda i: np.float64(quad([p + e for p, e in zip(x0, b[i])])), np.float64(quad(x0)), np.float64)
    assert abs(lap - want) <= 256 * EPS      # sums of magnitude up to 20 |field| ~ 1000
    # the gradient of the quadratic field at x0 (centred differences are exact on quadratics)
    if grid.dim == 3:
        g_want = [4.0 * x0[0] + x0[1] + a[0], 6.0 * x0[1] + x0[0] - 2.0 * x0[2] + a[1], -2.0 * x0[2] - 2.0 * x0[1] + a[2]]
    else:
        g_want = [4.0 * x0[0] + x0[1] + a[0], 6.0 * x0[1] + x0[0] + a[1]]
    assert all(abs(g - gw) <= 64 * EPS for g, gw in zip(grad, g_want))


def flat_interfaces(shape=FLAT['shape'], kappa=FLAT['kappa'], A=FLAT['A'], **_):
    ny, nx = shape
    xi = np.sqrt(2.0 * kappa / A)
    x = np.arange(nx, dtype=np.float64)
    profile = np.tanh((x - (nx / 4 - 0.5)) / xi) - np.tanh((x - (3 * nx / 4 - 0.5)) / xi) - 1.0
    return np.tile(profile, (ny, 1))


def test_flat_interfaces_stay_tanh_profiles():
    """D2Q9, 64 x 8, periodic, two flat interfaces phi = tanh(x / sqrt(2 kappa / A)), kappa = A = 0.04, tau_a = tau_b =
    tau_phi = 1, Gamma = 0.5, float64, 2000 steps.  Measured with this twin: the profile's largest deviation from the tanh
    it started as 3.533e-02 (the discrete equilibrium profile of an interface 1.4 nodes wide is not the continuum one),
    largest |v| 1.093e-07 (the profile is still settling along x; nothing moves along y), the sum of phi over the box moves
    by 6.6e-14 = 0.6 N eps.  Asserted with a margin of 2 over the two measured values; the figures are in profiles/NOTES.md."""
    c = dict((k, FLAT[k]) for k in ('kappa', 'A', 'tau_a', 'tau_b', 'tau_phi', 'Gamma'))
    phi0 = flat_interfaces()
    t = tw.FeTwin(sym.D2Q9, FLAT['shape'], np.float64, **c)
    zero = np.zeros(FLAT['shape'])
    t.set_fields(np.ones(FLAT['shape']), phi0, [zero, zero])
    s0 = float(tw.density(t.g).sum())
    t.run(FLAT['steps'])
    t.macro()
    dev = float(np.max(np.abs(t.phi - phi0)))
    vmax = float(max(np.max(np.abs(c)) for c in t.v))
    drift = abs(float(t.phi.sum()) - s0)
    print('flat interfaces: deviation from tanh %.3e, max |v| %.3e, drift of sum(phi) %.3e' % (dev, vmax, drift))
    assert np.all(np.isfinite(t.phi))
    assert dev <= 2 * 3.533e-2
    assert vmax <= 2 * 1.093e-7
    assert np.max(np.abs(t.phi - t.phi[:1])) <= 64 * EPS          # stays flat
    # every step changes a node's phi by the rounding of Q updates and a Q-term sum: N nodes, a few eps each, random signs
    assert drift <= phi0.size * EPS


def test_order_parameter_is_conserved_on_a_random_box():
    """sum(phi) over a periodic box is constant to N eps (collisions conserve each node's phi to the rounding of its Q
    updates, streaming moves values): D3Q19 12 x 6 x 5, 30 steps, random smooth phi."""
    shape = (5, 6, 12)
    rng = np.random.RandomState(5)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    phi0 = 0.8 * np.sin(2 * np.pi * x / shape[2] + 0.3) * np.cos(2 * np.pi * y / shape[1]) + 0.1 * np.sin(2 * np.pi * z / shape[0])
    phi0 += 0.01 * rng.uniform(-1, 1, shape)
    t = tw.FeTwin(sym.D3Q19, shape, np.float64, kappa=0.03, A=0.04, tau_a=1.3, tau_b=0.8, Gamma=0.6, tau_phi=0.9)
    zero = np.zeros(shape)
    t.set_fields(np.ones(shape), phi0, [zero, zero, zero])
    s0, m0 = float(t.g.sum()), float(t.f.sum())
    t.run(30)
    n = phi0.size
    assert abs(float(t.g.sum()) - s0) <= n * EPS and abs(float(t.f.sum()) - m0) <= n * EPS * 2
    assert np.max(np.abs(t.v[0])) > 1e-6          # the interface forces drive a flow: the run is not trivial
