"""The shallow-water model, host layer: LBFreeSurface's class surface, the descriptor it fills, what it refuses by name before
anything is built, its forcing through LBForcedSim, and the host stack -- controller, runner, halo exchange, AB and AA --
on the numpy twin behind the CPU test backend (tests/_sw_backend.py): one subdomain equals two, bit for bit.  No GPU."""
import argparse

import numpy as np
import pytest

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish_amd import hipabi
from sailfish_amd import node_type as nt
from sailfish_amd.lb_base import LBForcedSim, LBSim
from sailfish_amd.node_type import DynamicValue
from sailfish_amd.sym import S
from tests import _sw
from tests._lat import merged
from tests.test_accf_host import real_and_rest, runners_of

CPU = dict(gpus=[0], backends='tests._sw_backend')


def test_the_reference_import_works():
    from sailfish.lb_single import LBFluidSim, LBFreeSurface
    assert issubclass(LBFreeSurface, LBFluidSim) and not issubclass(LBFreeSurface, LBForcedSim)
    doc = LBFreeSurface.__doc__
    assert 'water depth' in doc and 'conserves' in doc


def test_class_surface():
    from sailfish.lb_single import LBFreeSurface
    p = argparse.ArgumentParser()
    LBFreeSurface.add_options(p, 2)
    assert p.parse_args([]).gravity == 0.001 and p.parse_args(['--gravity=0.05']).gravity == 0.05
    cfg = argparse.Namespace(grid='D3Q19', model='bgk')
    LBFreeSurface.modify_config(cfg)
    assert (cfg.grid, cfg.model) == ('D2Q9', 'bgk')                        # --grid=D3Q19 is overridden, as in the reference
    for model in ('mrt', 'elbm'):
        with pytest.raises(NotImplementedError, match='--model=%s' % model):
            LBFreeSurface.modify_config(argparse.Namespace(grid='D2Q9', model=model))


def test_constants_and_descriptor():
    _, (r,) = runners_of(_sw.make_sim(), 2, 'LBGeometry2D', _sw.config((12, 6), gravity=0.03, grid='D3Q19'))
    sim = r._sim
    assert sim.constants()['gravity'] == 0.03 and sim.grid.__name__ == 'D2Q9'
    d = r._module_desc()
    assert (d.equilibrium, d.gravity, d.lattice, d.model) == (hipabi.SLF_EQ_SHALLOW_WATER, _sw.g32(0.03), hipabi.SLF_D2Q9, hipabi.SLF_BGK)
    assert d.incompressible == hipabi.SLF_DENSITY_COMPRESSIBLE and d.has_force == 0 and d.accel_field == 0
    assert d.struct_size == hipabi.ctypes.sizeof(hipabi.SlfModuleDesc)
    assert not hasattr(sim, 'get_resident_kernels')                      # the runner asks with hasattr
    # every other simulation's descriptor carries the polynomial
    from sailfish_amd.lb_single import LBFluidSim
    _, (r,) = runners_of(_sw.make_sim(base=LBFluidSim), 2, 'LBGeometry2D', dict(_sw.config((12, 6)), gravity=None))
    d = r._module_desc()
    assert d.equilibrium == hipabi.SLF_EQ_BGK and d.gravity == 0.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------

BASE = dict(lattice=hipabi.SLF_D2Q9, model=hipabi.SLF_BGK, type_kind=[0, 1, 4, 5, hipabi.SLF_NK_SLIP],
            equilibrium=hipabi.SLF_EQ_SHALLOW_WATER, gravity=0.05)
DESC_REFUSALS = [
    (dict(model=hipabi.SLF_MRT), '--model=mrt'),
    (dict(model=hipabi.SLF_ELBM), '--model=elbm'),
    (dict(regularized=1), '--regularized'),
    (dict(subgrid=1), '--subgrid'),
    (dict(incompressible=hipabi.SLF_DENSITY_ROUNDOFF), '--minimize_roundoff'),
    (dict(incompressible=hipabi.SLF_DENSITY_INCOMPRESSIBLE), '--incompressible'),
    (dict(node_addressing=hipabi.SLF_ADDR_INDIRECT), '--node_addressing=indirect'),
    (dict(type_kind=[0, 1, hipabi.SLF_NK_EQUILIBRIUM_DENSITY]), 'NTEquilibriumDensity'),
    (dict(type_kind=[0, 1, hipabi.SLF_NK_ZOUHE_VELOCITY]), 'NTZouHeVelocity'),
    (dict(type_kind=[0, 1, hipabi.SLF_NK_WALL_TMS]), 'NTWallTMS'),
    (dict(lattice=hipabi.SLF_D3Q19), 'D2Q9 only'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_SINGLE), 'single-fluid'),
]


@pytest.mark.parametrize('extra,word', DESC_REFUSALS, ids=[w for _, w in DESC_REFUSALS])
def test_check_module_desc_refuses_by_name(extra, word):
    from sailfish_amd.lb_single import LBFreeSurface
    LBFreeSurface.check_module_desc(dict(BASE))                                    # the served base case
    LBSim.check_shallow_water(dict(BASE, equilibrium=0, **extra))                  # the polynomial: not this refusal's business
    with pytest.raises(NotImplementedError) as e:
        LBFreeSurface.check_module_desc(dict(BASE, **extra))
    assert 'shallow water' in str(e.value) and word in str(e.value)


def test_gravity_must_be_positive():
    with pytest.raises(ValueError, match='--gravity must be positive'):
        LBSim.check_shallow_water(dict(BASE, gravity=0.0))


@pytest.mark.parametrize('cfg,walls,word', [
    (dict(regularized=True), None, '--regularized'), (dict(subgrid='les-smagorinsky'), None, '--subgrid'),
    (dict(minimize_roundoff=True), None, '--minimize_roundoff'), (dict(incompressible=True), None, '--incompressible'),
    (dict(node_addressing='indirect'), None, '--node_addressing=indirect'),
    (dict(), nt.NTEquilibriumDensity(1.0), 'NTEquilibriumDensity'), (dict(), nt.NTWallTMS, 'NTWallTMS')],
    ids=lambda v: v if isinstance(v, str) else '')
def test_runner_refuses_before_anything_is_built(cfg, walls, word):
    _, (r,) = runners_of(_sw.make_sim(walls=walls), 2, 'LBGeometry2D', dict(_sw.config((12, 6), walls=walls), **cfg))
    with pytest.raises(NotImplementedError) as e:
        r._module_desc()
    assert 'shallow water' in str(e.value) and word in str(e.value)


# ---- forcing ------------------------------------------------------------------------------------------------------------------

def test_forces_through_lbforcedsim():
    from sympy import sin
    forces = [(1e-5, -2e-5), DynamicValue(1e-6 * sin(S.time), 0.0), DynamicValue(3e-5 * sin(0.5 * S.gx), 1e-6 * S.gy)]
    _, (r,) = runners_of(_sw.make_sim(forces=forces), 2, 'LBGeometry2D',
                         dict(_sw.config((12, 6)), force_implementation='edm'))
    sim = r._sim
    assert sim.has_accel_field and sim.time_dependent_force
    d = r._module_desc()
    assert (d.equilibrium, d.accel_field, d.has_force, d.force_implementation) == (1, 1, 1, hipabi.SLF_FORCE_EDM)
    assert list(d.accel)[:2] == [1e-5, -2e-5]
    real, rest = real_and_rest(r, r.accel_field_host())
    hy, hx = np.mgrid[0:6, 0:12].astype(np.float64)
    assert np.allclose(real[0], 3e-5 * np.sin(0.5 * hx), rtol=1e-12, atol=1e-20) and np.allclose(real[1], 1e-6 * hy, rtol=1e-12)
    assert np.all(rest == 0)
    # accel=False and grid != 0 stay refused
    plain = _sw.make_sim()(r.config)
    with pytest.raises(NotImplementedError, match='accel=True'):
        plain.add_body_force(DynamicValue(1e-5 * S.gx, 0.0), accel=False)
    with pytest.raises(NotImplementedError, match='grid=0'):
        plain.add_body_force(DynamicValue(1e-5 * S.gx, 0.0), grid=1)


def test_a_force_of_position_reaches_set_accel_field_and_no_resident_path():
    from tests import _sw_backend
    del _sw_backend.LOG[:]
    sim = _sw.make_sim(forces=[DynamicValue(3e-5 * S.gx, 0.0)])
    ctrl = _sw.run(sim, _sw.config((12, 6), precision='single'), 6, **CPU)
    (r,) = ctrl.runners
    log = list(_sw_backend.LOG)
    kinds = [e[0] for e in log]
    assert log[0] == ('build', 1, _sw.g32(0.05))
    assert kinds.count('set_accel_field') == 1 and kinds.index('set_accel_field') < kinds.index('run')
    _, module, addr, field = log[kinds.index('set_accel_field')]
    assert module is r.module and addr == r._gpu_accel_field
    host = r.accel_field_host()
    assert np.array_equal(field.reshape(host.shape), host) and np.ptp(field) > 0
    names = [e[1] for e in log if e[0] in ('get_kernel', 'run')]
    assert 'CollideAndPropagateResident' not in names
    assert [e[1] for e in log if e[0] == 'run'].count('CollideAndPropagate') == 6          # one launch per step
    assert r._resident_setup() is None
    # ... nor without a force: the small periodic box every other 2-D class would run several steps per launch on
    del _sw_backend.LOG[:]
    ctrl = _sw.run(_sw.make_sim(), _sw.config((12, 6), precision='single'), 6, **CPU)
    names = [e[1] for e in _sw_backend.LOG if e[0] in ('get_kernel', 'run')]
    assert 'CollideAndPropagateResident' not in names and ctrl.runners[0]._resident_setup() is None


# ---- the host stack on the twin -------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def whole():
    """24 x 12, slip-free: half-way walls on the y faces would pin the cut along y to a wall, so the box is periodic; the
    hump off centre plus a position-dependent force break every symmetry.  One subdomain, per pattern, computed once."""
    out = {}
    for pattern in ('AB', 'AA'):
        ctrl = _sw.run(SPLIT_SIM, _sw.config((24, 12), pattern=pattern), 9, **CPU)
        out[pattern] = dict((w, merged(ctrl, w)) for w in ('dist', 'rho', 'v0', 'v1'))
    return out


SPLIT_SIM = _sw.make_sim(forces=[(1e-5, 2e-5), DynamicValue(2e-5 * S.gx, -1e-5 * S.gy)])


@pytest.mark.parametrize('axis,cut', [(0, 11), (1, 5)], ids=['x', 'y'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_one_subdomain_equals_two_bit_for_bit(whole, pattern, axis, cut):
    ctrl = _sw.run(SPLIT_SIM, _sw.config((24, 12), pattern=pattern), 9, geo=_sw.strip_geometry(axis, cut), **CPU)
    assert len(ctrl.runners) == 2
    for w in ('dist', 'rho', 'v0', 'v1'):
        got = merged(ctrl, w)
        assert np.all(np.isfinite(got)) and np.array_equal(got, whole[pattern][w]), w
    assert np.ptp(whole[pattern]['rho']) > 0.05


def test_runner_on_the_twin_equals_the_bare_model():
    """What the host stack adds to the twin is data movement: 8 steps of the runner equal the np.roll box."""
    from tests import _sw_twin as tw
    ctrl = _sw.run(_sw.make_sim(), _sw.config((24, 12)), 8, **CPU)
    h, v = _sw.global_fields((12, 24))
    want = tw.model(24, 12, _sw.g32(0.05), 0.01, h, 8, v=v)
    assert np.array_equal(merged(ctrl, 'dist'), want)
