"""The numpy twin of the temperature lattice (tests/_thermal_twin.py) against what the model must do: heat
is conserved in an adiabatic box, conduction between plates gives the straight line through the link mid-points, a sine
wave in a uniform flow decays and travels as the advection-diffusion equation says, and a layer heated from below is
stable below the critical Rayleigh number and unstable above it.  The figures measured here are the bounds of the GPU tests
(tests/test_gpu_thermal.py allows twice the twin's error).  No GPU."""
import numpy as np
import pytest

from sailfish_amd import sym
from sailfish_amd.box import make_box_desc
from tests import _accf, _thermal
from tests._thermal_twin import ThermalTwinBox, lattice, tau_of

# measured with the double-precision twin (printed by the tests below)
WAVE_L2, WAVE_RATE, WAVE_SPEED = 1.8557e-3, 5.753e-3, 1.83e-8       # relative errors, magnitudes
WAVE_SPEED_F32 = 1.02e-6            # the phase-speed error of the SINGLE-precision twin: rounding, not discretisation


def test_lattice_constants():
    for dim, (q, k, w0) in ((2, (5, 3.0, 1.0 / 3.0)), (3, (7, 4.0, 0.25))):
        Q, w, kk = lattice(dim)
        assert (Q, kk, w[0]) == (q, k, w0) and abs(sum(w) - 1.0) < 1e-15
        assert abs(sum(w[1:3]) * kk - 1.0) < 1e-15                  # sum_i w_i e_ia e_ib = delta_ab / k
        assert abs((tau_of(0.1, dim) - 0.5) / kk - 0.1) < 1e-15


# ---- (a) heat conservation --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dim', [2, 3])
def test_heat_is_conserved_exactly_at_rest(dim):
    """Closed box -- no axis periodic, no node map: the faces bounce back --, u = 0, b = 0, double precision: sum(T) moves
    by less than n eps sum(T) over 200 steps (each step's T is a sum of the populations as streamed: nothing is lost, the
    difference is the rounding of the collisions)."""
    size = (13, 7) if dim == 2 else (13, 7, 5)
    desc = make_box_desc(_thermal.GRIDS[dim], size, precision='double', access_pattern='AB', accel_field=True)
    shape = tuple(reversed(size))
    sim = ThermalTwinBox(desc, (False,) * 3, None, _thermal.start_temperature(size), None, 0.8, 0.0, [0.0] * dim)
    sim.set_fields(np.ones(shape), [np.zeros(shape)] * dim)
    sim.t.init(sim.v)
    total0 = sim.temperature().sum()
    for _ in range(200):
        sim.lattice_step()
    n = int(np.prod(size))
    drift = abs(sim.temperature().sum() - total0)
    print('heat at rest, %d-D: drift %.3e of %.6f (n eps sum = %.3e)' % (dim, drift, total0, n * np.finfo(float).eps * total0))
    assert drift <= n * np.finfo(float).eps * total0
    assert np.ptp(sim.temperature()) < 0.4                          # and it diffuses


def test_heat_is_conserved_in_a_stirred_adiabatic_channel():
    """The coupled run: adiabatic full-way walls (wall_temperature NaN), periodic along x, a seeded flow and buoyancy.  The
    collision conserves sum_i g_i (sum_i geq_i = T: opposite directions cancel), so sum(T) over the wet nodes stays within
    the rounding of steps x nodes operations."""
    size = (24, 12)
    desc, periodic, map_fn = _accf.box_desc(sym.D2Q9, size, 'AB', 'double', 'guo', 'full', 1, accel_field=True)
    sim = ThermalTwinBox(desc, periodic, map_fn(desc), _thermal.start_temperature(size), None, 0.7, 0.5, [0.0, 1e-3])
    _accf.start(sim, size, 2)
    wet = sim.t.wet[0, 1:-1, 1:size[0] + 1]
    total0 = sim.temperature()[wet].sum()
    steps = 100
    for _ in range(steps):
        sim.step()
    drift = abs(sim.temperature()[wet].sum() - total0)
    print('heat, stirred channel: drift %.3e of %.6f' % (drift, total0))
    assert drift <= steps * wet.sum() * np.finfo(float).eps
    assert np.abs(sim.velocity()[1][wet]).max() > 1e-3              # the fluid moves
    assert sim.t.T[0, 1, 1] == _thermal.start_temperature(size)[0, 0]          # wall nodes are not written


# ---- (b) pure conduction ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tau_t,H,steps', _thermal.CONDUCTION)
def test_conduction_profile_is_the_straight_line_through_the_link_mid_points(tau_t, H, steps):
    """Plates at Tw = 1 and Tw = 0, u = 0.  With g_neq = -tau_T w_i e_i . grad T the anti-bounce-back rule gives
    Tw = T_b + 1/2 e . grad T for every tau_T: the steady profile is exact, T_j = 1 - (j - 1/2) / H.  Asserted to 100 eps;
    measured 40.5, 60 and 3 eps for the three cases (the rounding of thousands of steps, not a discretisation error)."""
    dev = _thermal.conduction(_thermal.twin_box, 'double', tau_t, H, steps)
    print('conduction, tau_T = %g, H = %d: %.1f eps' % (tau_t, H, dev))
    assert dev <= 100.0


# ---- (c) advected sine wave ---------------------------------------------------------------------------------------------------------

def test_advected_sine_wave_decays_and_travels():
    """70 x 8 periodic, u = (0.05, 0), kappa = 0.1, T = 0.5 + 0.1 sin(2 pi x / 70), 400 steps.  Measured with the double-
    precision twin: the decay rate is 0.575 % below kappa k^2, the phase speed 1.8e-8 below u, and the perturbation differs
    from 0.1 exp(-kappa k^2 t) sin(k (x - u t)) by 1.8557e-3 in the relative L2 norm (all of it the decay rate: the lattice's
    fourth-order diffusion error).  The asserted windows only pin those measurements down; the GPU tests take twice them."""
    l2, rate, speed = _thermal.advected_wave(_thermal.twin_box, 'double')
    print('advected wave (twin, double): relative L2 error %.4e, decay rate error %.4e, phase speed error %.4e' % (l2, rate, speed))
    assert abs(l2 / WAVE_L2 - 1.0) < 1e-2
    assert abs(abs(rate) / WAVE_RATE - 1.0) < 1e-2
    assert abs(speed) <= 1.01 * WAVE_SPEED


def test_advected_sine_wave_phase_speed_in_single_precision():
    """The same wave through the single-precision twin.  Its fitted phase speed is 1.02e-6 above u -- fifty times the double
    twin's error and all of it rounding: T = 0.5 +- 0.1 is stored to 3e-8, 400 times over.  The device computes the twin's
    bits, so this figure, not the double twin's 1.8e-8, is what its single-precision phase speed can be held to
    (tests/test_gpu_thermal.py allows twice it).  L2 error and decay rate stay within twice the double twin's."""
    l2, rate, speed = _thermal.advected_wave(_thermal.twin_box, 'single')
    print('advected wave (twin, single): relative L2 error %.4e, decay rate error %.4e, phase speed error %.4e' % (l2, rate, speed))
    assert abs(speed) <= 1.01 * WAVE_SPEED_F32 and abs(speed) >= 0.5 * WAVE_SPEED_F32
    assert l2 <= 2.0 * WAVE_L2 and abs(rate) <= 2.0 * WAVE_RATE


# ---- (d) Rayleigh-Benard onset ------------------------------------------------------------------------------------------------------

def test_rayleigh_benard_onset():
    """32 x 18 (H = 16) between full-way walls, Pr = 1, nu = kappa = 0.03, a seeded roll pair of amplitude 1e-3, 2000 steps.
    Measured with the double-precision twin: KE(2000) / KE(1000) = 76.6 at Ra = 5000 and 0.112 at Ra = 800 (critical:
    1707.76), peak speed 3.7e-3.  Asserted: the factor-2 bounds of the issue and nothing tighter."""
    growth, peak_above = _thermal.rayleigh_benard(_thermal.twin_box, 'double', _thermal.RB['above'])
    decay, peak_below = _thermal.rayleigh_benard(_thermal.twin_box, 'double', _thermal.RB['below'])
    print('Rayleigh-Benard (twin, double): KE ratio %.3f at Ra = 5000 (peak %.3e), %.4f at Ra = 800 (peak %.3e)'
          % (growth, peak_above, decay, peak_below))
    assert growth >= 2.0 and decay <= 0.5
    assert max(peak_above, peak_below) < 0.1
