"""Flow statistics without a GPU: the numpy twin of the kernels (tests/_stats_twin.py) and the host functions of
sailfish_amd/util.py against what the reference's util.vorticity / kinetic_energy / enstrophy returned for the Kida
field (tests/golden/flow_stats.npz, tools/capture_stats_goldens.py), and the public surface of sailfish.stats."""
import os

import numpy as np
import pytest

from tests import _host
from tests import _stats_twin as tw

PRECISIONS = [('f32', np.float32), ('f64', np.float64)]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'flow_stats.npz'))


@pytest.mark.parametrize('tag,dtype', PRECISIONS)
def test_twin_stencil_equals_the_reference_vorticity(golden, tag, dtype):
    v = golden['v_' + tag]
    assert v.dtype == dtype and v.shape == (3, 9, 12, 20)
    assert np.array_equal(v, tw.kida(tuple(golden['size']), float(golden['max_v']), dtype))
    w = tw.vorticity(v)
    assert w.dtype == dtype
    assert np.array_equal(w, golden['vorticity_' + tag])


@pytest.mark.parametrize('tag,dtype', PRECISIONS)
def test_util_functions_reproduce_the_reference(golden, tag, dtype):
    from sailfish_amd import util
    v = golden['v_' + tag]
    w = util.vorticity(v, 1.0)
    assert w.dtype == dtype and np.array_equal(w, golden['vorticity_' + tag])
    assert np.array_equal(util.vorticity(v), w)                 # dx defaults to 1
    n = v[0].size
    # the two scalars: sums of n (3 n) terms, then one division
    for got, want, terms in ((util.kinetic_energy(v), golden['kinetic_energy_' + tag], np.square(v)),
                             (util.enstrophy(v, 1.0), golden['enstrophy_' + tag], np.square(w))):
        _, bound = tw.sum_and_bound(terms, divisions=1, divisor=2.0 * n)
        print('%s: %.17g vs reference %.17g, bound %.3e' % (tag, got, float(want), bound))
        assert abs(float(got) - float(want)) <= bound
    if dtype is np.float64:
        assert abs(float(golden['kinetic_energy_f64']) - 3.0 / 8.0 * 0.05 ** 2) < 1e-15


def test_twin_sums_agree_with_the_reference_scalars(golden):
    """The twin's v_sq / vort_sq, summed exactly, are the reference's energy and enstrophy up to the rounding of the
    reference's own numpy sums (double: pairwise, far inside n 2^-53 sum|t|)."""
    v = golden['v_f64']
    v_sq, vort_sq = tw.ke_fields(v)
    n = v[0].size
    for field, key in ((v_sq, 'kinetic_energy_f64'), (vort_sq, 'enstrophy_f64')):
        res, bound = tw.sum_and_bound(field, divisions=1, divisor=2.0 * n)
        # (the per-node sum of three squares adds two roundings per node to the reference's plain sum of squares)
        assert abs(res - float(golden[key])) <= bound + 3 * tw.U * abs(res)


def test_stats_alias_resolves_to_this_package():
    from sailfish.stats import FlowStatsMixIn, KineticEnergyEnstrophyMixIn, ReynoldsStatsMixIn
    import sailfish_amd.stats as st
    from sailfish_amd.lb_base import LBMixIn
    assert KineticEnergyEnstrophyMixIn is st.KineticEnergyEnstrophyMixIn
    assert ReynoldsStatsMixIn is st.ReynoldsStatsMixIn
    assert issubclass(KineticEnergyEnstrophyMixIn, FlowStatsMixIn) and issubclass(FlowStatsMixIn, LBMixIn)
    assert ReynoldsStatsMixIn.stat_buf_size == 1024
    assert 'snapshot_iters' not in vars(ReynoldsStatsMixIn)       # per instance, not shared between simulations
    assert st.PROFILE_KEYS == tw.PROFILE_KEYS and len(st.PROFILE_KEYS) == 22
    for name in ('compute_ke_enstropy', 'before_main_loop', 'fields'):
        assert hasattr(KineticEnergyEnstrophyMixIn, name)
    for name in ('prepare_reynolds_stats', 'collect_reynolds_stats'):
        assert hasattr(ReynoldsStatsMixIn, name)


def _sim_classes():
    from sailfish.lb_single import LBFluidSim
    from sailfish.stats import KineticEnergyEnstrophyMixIn, ReynoldsStatsMixIn

    class EnergySim(LBFluidSim, KineticEnergyEnstrophyMixIn):
        pass

    class ProfileSim(LBFluidSim, ReynoldsStatsMixIn):
        pass
    return EnergySim, ProfileSim


def test_mixin_declares_its_fields():
    from sailfish_amd.lb_base import ScalarField
    EnergySim, ProfileSim = _sim_classes()
    declared = EnergySim(_host.make_config(3))._declared_fields()
    names = [f.name for f in declared]
    assert names.count('v_sq') == 1 and names.count('vort_sq') == 1 and 'rho' in names and 'v' in names
    for f in declared:
        if f.name in ('v_sq', 'vort_sq'):
            assert isinstance(f, ScalarField) and f.gpu_array and f.init == 0.0
    assert 'v_sq' not in [f.name for f in ProfileSim(_host.make_config(3))._declared_fields()]


def test_two_dimensional_simulations_are_refused():
    EnergySim, ProfileSim = _sim_classes()
    from sailfish.stats import KineticEnergyEnstrophyMixIn
    with pytest.raises(NotImplementedError, match='3-D'):           # (the hook as the runner calls it for a mix-in)
        KineticEnergyEnstrophyMixIn.before_main_loop(EnergySim(_host.make_config(2)), None)
    with pytest.raises(NotImplementedError, match='3-D'):
        ProfileSim(_host.make_config(2)).prepare_reynolds_stats(None)


def test_kida_example_initial_field_is_the_fixture(golden):
    from examples.kida_vortex import KidaSim, KidaSubdomain, kida_velocity
    nx, ny, nz = [int(n) for n in golden['size']]
    hz, hy, hx = np.mgrid[0:nz, 0:ny, 0:nx]
    v = kida_velocity(hx * np.pi * 2.0 / nx, hy * np.pi * 2.0 / ny, hz * np.pi * 2.0 / nz, KidaSubdomain.max_v)
    assert np.array_equal(np.array(v), golden['v_f64'])
    assert issubclass(KidaSim, __import__('sailfish_amd.stats', fromlist=['x']).KineticEnergyEnstrophyMixIn)
