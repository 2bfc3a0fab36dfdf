"""Two refusals of slf_kernel_launch on the device, with the code and the text that the CPU record holds for them
(tests/golden/abi_launch.tsv, section `launch`; tests/test_abi_bind.py): an in-place (AA) CollideAndPropagate bound
without the iteration flag, and a kernel armed for the pair sweep launched with a region.  Nothing is written by either.

Only refusals that are harmless if the check were wrong are tried here: the first would run an even step, the second a
whole-box pair step.  Regions outside the real nodes, NULL node maps, NULL node tables and an unset acceleration field
are NOT tried on a GPU: against a broken check they would be wild loads and stores.  The CPU record covers them.

The AA module is 8 x 6 x 5.  The pair sweep serves rows of 64 .. 512 nodes only (slf_kernel_set_pair refuses shorter
ones), so the armed kernel belongs to the smallest box that can be armed, 64 x 6 x 5."""
import os

import numpy as np
import pytest

from sailfish_amd import sym
from sailfish_amd.box import BoxSim, make_box_desc

pytestmark = pytest.mark.gpu
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'abi_launch.tsv')


def _recorded(config, what):
    """(code, message) of the launch of CollideAndPropagate in `config`, try `what`"""
    for ln in open(RECORD):
        section, subject, cfg, name, code, message, _ = ln.rstrip('\n').split('\t')
        if (section, subject, cfg, name) == ('launch', 'CollideAndPropagate', config, what):
            return int(code), message
    raise KeyError((config, what))


def _backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def _refused(b, kernel, region, stream, config, what):
    code, message = _recorded(config, what)
    assert code != 0 and message
    with pytest.raises(b.FatalError) as err:
        b.run_kernel(kernel, region, stream)
    assert '(status %d): %s' % (code, message) in str(err.value), (str(err.value), code, message)


def test_aa_sweep_without_the_iteration_flag_is_refused_and_writes_nothing():
    b = _backend()
    sim = BoxSim(b, make_box_desc(sym.D3Q19, (8, 6, 5), precision='single', access_pattern='AA', visc=0.02))
    f = np.random.RandomState(1).rand(19, *sim.shape).astype(sim.dtype)
    sim.set_dist(f)
    args = [sim.gpu_map, sim.gpu_dist[0], sim.gpu_dist[0], sim.gpu_rho] + sim.gpu_v + [0]
    k = b.get_kernel(sim.module, 'CollideAndPropagate', (64,), args, 'P' * 7 + 'i', needs_iteration=False)
    for region in (None, (1, 3, 1, 2)):
        _refused(b, k, region, sim.stream, 'bgk-d3q19-aa-direct', 'no-iteration')
    assert np.array_equal(sim.get_dist(), f)
    sim.release()


def test_pair_armed_kernel_with_a_region_is_refused_and_writes_nothing():
    b = _backend()
    desc = make_box_desc(sym.D3Q19, (64, 6, 5), precision='single', access_pattern='AB', visc=0.02, periodic_fused=[1, 1, 1])
    sim = BoxSim(b, desc, periodic=(True, True, True))
    assert sim.k_pair is not None, sim.pair_refused
    rng = np.random.RandomState(2)
    f = [rng.rand(19, *sim.shape).astype(sim.dtype) for _ in range(2)]
    for which in (0, 1):
        sim.set_dist(f[which], which=which)
    _refused(b, sim.k_pair[0], (1, 3, 1, 2), sim.stream, 'bgk-d3q19-ab-fluid-only', 'pair-armed-region')
    for which in (0, 1):
        assert np.array_equal(sim.get_dist(which=which), f[which])
    sim.release()
