"""examples/binary_fluid/fe_separation_2d.py (at 64^2) and fe_separation_3d.py (at its default 32^3) through
LBSimulationController: 200 steps, finite results, the order parameter conserved, and the separation under way -- the
variance of phi moves the way it moves in the numpy twin's run of the same seed."""
import importlib

import numpy as np
import pytest

from sailfish_amd import sym
from tests import _fe_twin as tw

pytestmark = pytest.mark.gpu

STEPS = 200


def _twin_variance_ratio(grid, shape, seed, defaults):
    noise = np.random.RandomState(seed).rand(*shape) / 100.0
    t = tw.FeTwin(grid, shape, np.float32, **dict((k, defaults[k]) for k in ('kappa', 'Gamma', 'A', 'tau_a', 'tau_b', 'tau_phi')))
    zero = np.zeros(shape)
    t.set_fields(np.ones(shape), noise, [zero] * grid.dim)
    v0 = float(np.var(noise))
    t.run(STEPS - 1)
    t.macro()
    return float(np.var(t.phi.astype(np.float64))) / v0


@pytest.mark.parametrize('module,dim,size', [('fe_separation_2d', 2, (64, 64)), ('fe_separation_3d', 3, (32, 32, 32))])
def test_separation_examples(module, dim, size):
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    mod = importlib.import_module('examples.binary_fluid.' + module)
    defaults = {}
    mod.SeparationFESim.update_defaults(defaults)
    if dim == 3:
        assert (defaults['lat_nx'], defaults['lat_ny'], defaults['lat_nz']) == size
    cfg = dict(lat_nx=size[0], lat_ny=size[1], max_iters=STEPS, quiet=True, perf_stats_every=0, seed=1234)
    ctrl = LBSimulationController(mod.SeparationFESim, getattr(geo_mod, 'LBGeometry%dD' % dim), default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    r = ctrl.runners[0]
    phi, rho = r._sim.phi.astype(np.float64), r._sim.rho.astype(np.float64)
    assert np.all(np.isfinite(phi)) and np.all(np.isfinite(rho)) and all(np.all(np.isfinite(c)) for c in r._sim.v)
    shape = tuple(reversed(size))
    noise = np.random.RandomState(1234).rand(*shape) / 100.0
    n = noise.size
    # every collision conserves a node's phi to the rounding of its Q updates and Q-term sums (single precision, |phi| << 1
    # here: populations below 0.01)
    Q = r._sim.grid.Q
    assert abs(phi.sum() - noise.astype(np.float32).astype(np.float64).sum()) <= n * STEPS * (Q + 2) * 0.5 * np.finfo(np.float32).eps * 0.01
    ratio = float(np.var(phi)) / float(np.var(noise))
    twin = _twin_variance_ratio(sym.D2Q9 if dim == 2 else sym.D3Q19, shape, 1234, defaults)
    print('%s: var(phi) after %d steps / at start = %.4f (twin %.4f)' % (module, STEPS, ratio, twin))
    # (white noise first loses its short wavelengths to diffusion -- the variance falls in the twin over these 200 steps --
    # while the long ones grow.)  Twin and kernels do the same single-precision operations; what summation order may
    # differ by is 1e-7 per step on values of 0.01: the variances agree far inside a percent
    assert (ratio >= 1.0) == (twin >= 1.0)
    assert abs(ratio - twin) <= 0.01 * twin
