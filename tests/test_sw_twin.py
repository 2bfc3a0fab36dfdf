"""The numpy twin of the shallow-water model (tests/_sw_twin.py) against the reference's expression objects
(tests/golden/arith_sw_D2Q9.npz, tools/capture_sw.py) and against the physics: the moving populations are the reference's,
the rest population is the conserving one -- the reference's minus 2 h v^2, the stated difference of DESIGN.md §9i --, the
mass of a periodic box stays put and a gravity wave travels at sqrt(g h0).  No GPU."""
import os

import numpy as np
import pytest

from tests import _lat_twin as lt
from tests import _sw_twin as tw

EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'arith_sw_D2Q9.npz'))


def states(G):
    return G['h'].copy(), [G['v'][:, 0].copy(), G['v'][:, 1].copy()]


def test_fixture_is_what_the_issue_states(golden):
    G = golden
    assert list(G['gravity']) == [0.001, 0.05]
    assert G['h'].shape == (48,) and G['v'].shape == (48, 2) and G['feq'].shape == (2, 48, 9)
    assert G['h'].min() >= 0.5 and G['h'].max() <= 1.5 and np.ptp(G['h']) > 0.5
    speed = np.hypot(G['v'][:, 0], G['v'][:, 1])
    assert speed.max() <= 0.1 and speed[0] == 0 and speed.max() > 0.05


@pytest.mark.parametrize('k', [0, 1], ids=['g=0.001', 'g=0.05'])
def test_moving_populations_are_the_references(golden, k):
    """Populations 1..8 to the rounding of float64: the expression is some ten operations on values below 2 h w_i."""
    h, v = states(golden)
    fe = tw.sw_equilibrium(h, v, float(golden['gravity'][k]), np.float64)
    want = golden['feq'][k].T
    assert np.max(np.abs(fe[1:] - want[1:])) <= 16 * EPS * np.max(np.abs(want[1:]))


@pytest.mark.parametrize('k', [0, 1], ids=['g=0.001', 'g=0.05'])
def test_rest_population_is_the_references_minus_2hv2(golden, k):
    """The stated difference: the twin's (the kernels') rest population is Zhou's, the reference's exceeds it by 2 h v^2."""
    h, v = states(golden)
    g = float(golden['gravity'][k])
    fe = tw.sw_equilibrium(h, v, g, np.float64)
    ref0 = golden['feq'][k][:, 0]
    vsq = v[0] * v[0] + v[1] * v[1]
    assert np.max(np.abs(fe[0] - (ref0 - 2.0 * h * vsq))) <= 16 * EPS * np.max(h)
    assert np.max(2.0 * h * vsq) > 1e4 * EPS             # ... which the fixture's states can tell apart
    # Zhou's closed form of the same thing
    zhou = h - (4.0 / 9.0) * h * (1.875 * g * h + 1.5 * vsq)
    assert np.max(np.abs(fe[0] - zhou)) <= 16 * EPS * np.max(h)
    # and the twin's copy of the reference's rest population is the fixture's
    assert np.max(np.abs(tw.sw_rest_reference(h, v, g, np.float64) - ref0)) <= 16 * EPS * np.max(h)


@pytest.mark.parametrize('k', [0, 1], ids=['g=0.001', 'g=0.05'])
def test_moments_of_the_equilibrium(golden, k):
    h, v = states(golden)
    fe = tw.sw_equilibrium(h, v, float(golden['gravity'][k]), np.float64)
    rho, u = lt.macro(tw.GRID, fe, False, np.float64)
    assert np.max(np.abs(rho - h)) <= 4 * EPS * np.max(h)
    for d in range(2):
        assert np.max(np.abs(u[d] * rho - h * v[d])) <= 16 * EPS
    # the reference's populations sum to h + 2 h v^2
    ref = golden['feq'][k]
    vsq = v[0] * v[0] + v[1] * v[1]
    assert np.max(np.abs(ref.sum(axis=1) - (h + 2.0 * h * vsq))) <= 16 * EPS * np.max(h)


def cosine_box(L, ny=4, amp=0.01):
    x = np.arange(L, dtype=np.float64)
    return np.tile(1.0 + amp * np.cos(2.0 * np.pi * x / L), (ny, 1))


def test_mass_of_a_periodic_box_and_what_the_reference_would_do():
    """64 x 4, periodic, g = 0.05, visc = 0.01, a 1 % cosine in h, 600 steps: the mass of 256 is kept to 1e-10; with the
    reference's rest population it grows by more than half a unit."""
    h = cosine_box(64)
    f = tw.model(64, 4, 0.05, 0.01, h, 600)
    assert abs(float(f.sum()) - float(h.sum())) <= 1e-10
    f = tw.model(64, 4, 0.05, 0.01, h, 600, rest=tw.sw_rest_reference)
    assert float(f.sum()) - float(h.sum()) > 0.5


def test_gravity_wave_period():
    """The cosine mode of the 64 x 4 box oscillates with the period L / sqrt(g h0), from zero crossings, within 1 %."""
    L, g = 64, 0.05
    h = cosine_box(L)
    mode = np.cos(2.0 * np.pi * np.arange(L) / L)
    signal = []
    tw.model(L, 4, g, 0.01, h, 600, record=lambda t, f: signal.append(float((f.sum(axis=0)[0] * mode).sum())))
    period = tw.period_from_crossings(signal)
    theory = L / np.sqrt(g * 1.0)
    print('period %.3f, theory %.3f, relative difference %.2e' % (period, theory, period / theory - 1.0))
    assert abs(period / theory - 1.0) <= 0.01


def test_twin_box_equals_the_bare_model_bit_for_bit():
    """The twin behind the descriptor (ghost layers, in-sweep wrap, AB and AA) against the bare np.roll box."""
    from tests import _sw
    rng = np.random.RandomState(5)
    h = 1.0 + 0.1 * rng.rand(6, 10)
    v = [0.02 * (rng.rand(6, 10) - 0.5), 0.02 * (rng.rand(6, 10) - 0.5)]
    want = tw.model(10, 6, _sw.g32(0.05), 0.02, h, 4, v=v)       # (the descriptor carries the gravity in single precision)
    for pattern in ('AB', 'AA'):
        desc, periodic, _ = _sw.box_desc((10, 6), pattern, 'double', gravity=0.05, visc=0.02)
        box = tw.SwTwinBox(desc, periodic)
        box.set_fields(h, v)
        box.initial_conditions()
        box.run(4)
        assert np.array_equal(box.real_view(box.current_dist()), want[:, :, :]), pattern
