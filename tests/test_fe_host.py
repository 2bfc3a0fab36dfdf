"""Host side of the free-energy binary fluid (no GPU): options, module descriptor, kernel argument lists, what is refused
when a simulation is set up, the zero-gradient rims, and the exchange of phi in front of SetInitialConditions."""
import argparse
import ctypes

import numpy as np
import pytest

from sailfish_amd import hipabi, lb_base, lb_binary
from sailfish_amd import node_type as nt
from tests import _fe, _host, _sc
from tests.test_elbm_host import RecordingBackend


class LoggingBackend(RecordingBackend):
    """Records the names of the kernels that are launched, in order."""

    def __init__(self, *a, **kw):
        super(LoggingBackend, self).__init__(*a, **kw)
        self.launched = []

    def run_kernel(self, k, grid_size=None, stream=None):
        self.launched.append(k.name)


def _runners(sim_cls, dim, size, geo=None, **kw):
    cfg = _fe.config(dim, size, **kw) if issubclass(sim_cls, lb_binary.LBBinaryFluidFreeEnergy) else kw
    cfg_, specs, runners = _host.build_runners(sim_cls, dim, geo, cfg, backend_factory=LoggingBackend)
    return runners


def test_the_reference_import_path_and_option_defaults():
    import sailfish.lb_binary as alias
    assert alias.LBBinaryFluidFreeEnergy is lb_binary.LBBinaryFluidFreeEnergy
    p = argparse.ArgumentParser()
    for base in lb_binary.LBBinaryFluidFreeEnergy.mro():
        if 'add_options' in base.__dict__ and base is not lb_base.LBSim:
            base.add_options(p, 3)
    o = p.parse_args([])
    # reference lb_binary.py:159-176 and :33-35
    assert (o.bc_wall_grad_phase, o.bc_wall_grad_order, o.Gamma, o.kappa, o.A, o.tau_a, o.tau_b, o.model, o.tau_phi) == \
        (0.0, 2, 0.5, 0.5, 0.5, 1.0, 1.0, 'bgk', 1.0)
    with pytest.raises(SystemExit):
        p.parse_args(['--bc_wall_grad_order=3'])
    fields = lb_binary.LBBinaryFluidFreeEnergy.fields()
    assert [(type(f).__name__, f.name, f.need_nn) for f in fields] == [
        ('ScalarField', 'rho', False), ('ScalarField', 'phi', True), ('VectorField', 'v', False),
        ('ScalarField', 'phi_laplacian', False)]
    assert lb_binary.LBBinaryFluidFreeEnergy.nonlocality == 1


@pytest.mark.parametrize('dim,size', [(2, (24, 12)), (3, (20, 12, 10))])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_descriptor_and_kernel_argument_lists(dim, size, pattern):
    sim_cls, _ = _fe.make_sim(dim, walls=True)
    r = _runners(sim_cls, dim, size, pattern=pattern, walls=True, order=1, phase=0.1)[0]
    r.prepare()
    d = r.backend.desc
    assert d.struct_size == ctypes.sizeof(hipabi.SlfModuleDesc)
    assert d.simtype == hipabi.SLF_SIM_FREE_ENERGY == 3 and d.model == hipabi.SLF_BGK and d.has_force == 0
    P = _fe.PARAMS
    assert (d.fe_Gamma, d.fe_kappa, d.fe_A, d.fe_tau_a, d.fe_tau_b, d.tau_phi) == \
        (P['Gamma'], P['kappa'], P['A'], P['tau_a'], P['tau_b'], P['tau_phi'])
    assert (d.bc_wall_grad_phase, d.bc_wall_grad_order) == (0.1, 1)
    # x (and y in 3-D) periodic; the wall axis is neither periodic nor connected: its LOW rim only
    assert list(d.fe_zero_grad_rim) == ([0, 1, 0] if dim == 2 else [0, 0, 1])
    sim = r._sim
    assert sim.constants() == dict((k, P[k]) for k in ('Gamma', 'A', 'kappa', 'tau_a', 'tau_b'))
    v = r.gpu_field(sim.v)
    for kernels in (r._kernels_none, r._kernels_full):
        assert len(kernels) == 2
        for parity, (macro, sweeps) in enumerate(kernels):
            src = 0 if (pattern == 'AA' or parity == 0) else 1
            dst = 0 if pattern == 'AA' else 1 - src
            assert macro.name == 'FreeEnergyPrepareMacroFields' and macro.fmt == 'PPPPPi'
            assert macro.args[:5] == [r.gpu_geo_map(), r.gpu_dist(0, src), r.gpu_dist(1, src), r.gpu_field(sim.rho),
                                      r.gpu_field(sim.phi)]
            fluid, order = sweeps
            assert fluid.name == 'FreeEnergyCollideAndPropagateFluid' and fluid.fmt == 'P' * (6 + dim) + 'i'
            assert fluid.args[:-1] == [r.gpu_geo_map(), r.gpu_dist(0, src), r.gpu_dist(0, dst), r.gpu_field(sim.rho),
                                       r.gpu_field(sim.phi)] + v + [r.gpu_field(sim.phi_laplacian)]
            assert order.name == 'FreeEnergyCollideAndPropagateOrderParam' and order.fmt == 'P' * (5 + dim) + 'i'
            assert order.args[:-1] == [r.gpu_geo_map(), r.gpu_dist(1, src), r.gpu_dist(1, dst), r.gpu_field(sim.phi)] + v + \
                [r.gpu_field(sim.phi_laplacian)]
            assert fluid.args[-1] == order.args[-1] == macro.args[-1] == (3 if kernels is r._kernels_full else 2)
    assert r.backend.launched.count('SetInitialConditions') == (2 if pattern == 'AB' else 1)


class _Spec(object):
    X_LOW, X_HIGH, Y_LOW, Y_HIGH, Z_LOW, Z_HIGH = range(6)

    def __init__(self, periodic, connected):
        self._periodicity, self._conn = periodic, connected

    def has_face_conn(self, face):
        return face in self._conn


def test_zero_gradient_rims_mirror_the_reference_template():
    """mako_utils.mako:168-197 with its `%if ... %elif`: low rim where the axis is neither periodic nor connected on its
    low face; the high rim only when the low face IS connected and the high one is not."""
    rims = lb_binary.LBBinaryFluidFreeEnergy.zero_gradient_rims
    S = _Spec
    assert rims(S([False] * 3, ()), 3) == [1, 1, 1]
    assert rims(S([True, False, True], ()), 3) == [0, 1, 0]
    assert rims(S([False] * 3, (S.X_LOW, S.Y_HIGH, S.Z_LOW, S.Z_HIGH)), 3) == [2, 1, 0]
    assert rims(S([False] * 2, (S.X_HIGH,)), 2) == [1, 1, 0]          # high face connected, low one not: still the low rim
    assert rims(S([False, True], (S.X_LOW, S.X_HIGH)), 2) == [0, 0, 0]


class _HalfWalls(_fe.Subdomain2D):
    def boundary_conditions(self, hx, hy):
        self.set_node((hy == 0) | (hy == self.gy - 1), nt.NTHalfBBWall)

    def initial_conditions(self, sim, hx, hy):
        sim.rho[:] = 1.0


class _PressureWalls(_HalfWalls):
    def boundary_conditions(self, hx, hy):
        self.set_node(hy == 0, nt.NTEquilibriumDensity(1.0))


class _GuoWalls(_HalfWalls):
    def boundary_conditions(self, hx, hy):
        self.set_node(hy == 0, nt.NTGuoDensity(1.0))


def _sim_with(subdomain_cls, init=None):
    class Sim(lb_binary.LBBinaryFluidFreeEnergy):
        subdomain = subdomain_cls

        def __init__(self, config):
            super(Sim, self).__init__(config)
            if init:
                init(self)
    return Sim


PLAIN = _fe.make_sim(2)[0]
REFUSALS = [
    ('mrt', PLAIN, dict(model='mrt'), NotImplementedError, 'FE-MRT'),
    ('indirect', PLAIN, dict(node_addressing='indirect'), NotImplementedError, 'indirect'),
    ('minimize_roundoff', PLAIN, dict(minimize_roundoff=True), NotImplementedError, 'minimize_roundoff'),
    ('regularized', PLAIN, dict(regularized=True), NotImplementedError, 'regularized'),
    ('subgrid', PLAIN, dict(subgrid='les-smagorinsky'), NotImplementedError, 'subgrid'),
    ('incompressible', PLAIN, dict(incompressible=True), NotImplementedError, 'incompressible'),
    ('body force', _sim_with(PLAIN.subdomain, lambda s: s.add_body_force((1e-5, 0.0))), {}, NotImplementedError,
     'free_energy_external_force'),
    ('force for equilibrium', _sim_with(PLAIN.subdomain, lambda s: s.use_force_for_equilibrium(None, 1)), {},
     NotImplementedError, 'use_force_for_equilibrium'),
    ('half-way walls', _sim_with(_HalfWalls), dict(periodic_y=False), NotImplementedError, 'NTHalfBBWall'),
    ('other boundary types', _sim_with(_PressureWalls), dict(periodic_y=False), NotImplementedError, 'NTFullBBWall nodes only'),
    ('NTGuoDensity', _sim_with(_GuoWalls), dict(periodic_y=False), NotImplementedError, 'NTGuoDensity'),
]


@pytest.mark.parametrize('name,sim_cls,over,exc,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_when_the_simulation_is_set_up(name, sim_cls, over, exc, message):
    with pytest.raises(exc, match=message):
        r = _runners(sim_cls, 2, (24, 12), **over)[0]
        r.prepare()


def test_force_objects_are_refused():
    def add(sim):
        sim.add_force_oject(lb_base.ForceObject((3, 3), (5, 5)))
    with pytest.raises(NotImplementedError, match='force objects: single-fluid'):
        _runners(_sim_with(PLAIN.subdomain, add), 2, (24, 12))[0].prepare()


def test_order_two_wall_helper_outside_the_subdomain_is_refused():
    """Walls on the z faces, two subdomains along z of five layers each are fine (helper at z = 2 resp. 7); a wall whose
    order-2 helper lies beyond the seam is named."""
    from sailfish_amd import geo as geo_mod
    sim_cls, _ = _fe.make_sim(3, walls=True)
    for r in _runners(sim_cls, 3, (12, 8, 10), geo='EqualSubdomainsGeometry3D', walls=True, subdomains=2, conn_axis='z'):
        r.prepare()
    assert geo_mod.EqualSubdomainsGeometry3D is not None

    class Slab(_fe.Subdomain3D):           # a wall layer right under the seam of two subdomains along z, fluid above it
        def boundary_conditions(self, hx, hy, hz):
            self.set_node(hz == self.gz // 2 - 2, nt.NTFullBBWall)

        def initial_conditions(self, sim, hx, hy, hz):
            sim.rho[:] = 1.0

    with pytest.raises(ValueError, match=r'NTFullBBWall node \(0, 0, 3\).*outside subdomain 0'):
        for r in _runners(_sim_with(Slab), 3, (12, 8, 10), geo='EqualSubdomainsGeometry3D', walls=False, periodic_z=False,
                          subdomains=2, conn_axis='z'):
            r.prepare()
    # first order: the helper is the node next to the wall, inside
    for r in _runners(_sim_with(Slab), 3, (12, 8, 10), geo='EqualSubdomainsGeometry3D', walls=False, periodic_z=False,
                      subdomains=2, conn_axis='z', order=1):
        r.prepare()


def test_phi_is_exchanged_in_front_of_the_initial_conditions_of_free_energy_runners_only():
    """Ghost-layer periodic images of phi (the y axis here: --nohip_fused_periodic) and the pack kernels of the field
    exchange are launched before SetInitialConditions by a free-energy runner; a Shan-Chen runner launches neither."""
    from sailfish_amd.controller import LocalGroup
    sim_cls, _ = _fe.make_sim(2)
    r = _runners(sim_cls, 2, (24, 12), fused=False)[0]              # one subdomain: the periodic images only
    assert r._startup_needs_fields()
    r.prepare()
    log = r.backend.launched
    assert log[:log.index('SetInitialConditions')] == ['ApplyMacroPeriodicBoundaryConditions'] * 2
    runners = _runners(sim_cls, 2, (24, 12), geo='EqualSubdomainsGeometry2D', fused=False, subdomains=2, conn_axis='x')
    group = LocalGroup(runners)
    for r in runners:
        r.prepare()
    group._startup_fields()
    # (the group's queue performs every runner's entries through the first runner's backend)
    log = runners[0].backend.launched
    first = log.index('SetInitialConditions')
    for name in ('ApplyMacroPeriodicBoundaryConditions', 'CollectSparseData', 'DistributeSparseData'):
        assert log[:first].count(name) == 2, (name, log)
    assert 'SetInitialConditions' in runners[1].backend.launched
    for r in runners:
        # one field travels: phi (rho is not read at neighbouring nodes)
        assert r._macro_links and all(len(link.packs[0]) == 1 for link in r._macro_links.values())
    sc_cls, _ = _sc.make_sim(2)
    cfg = _sc.config(2, (24, 12), fused=False)
    cfg.update(subdomains=2, conn_axis='x')
    r = _host.build_runners(sc_cls, 2, 'EqualSubdomainsGeometry2D', cfg, backend_factory=LoggingBackend)[2][0]
    assert not r._startup_needs_fields()
    r.prepare()
    log = r.backend.launched
    assert log and set(log[:log.index('SetInitialConditions') + 1]) == {'SetInitialConditions'}


def test_runners_of_a_same_process_group_leave_the_start_up_to_the_group():
    from sailfish_amd.controller import LocalGroup
    sim_cls, _ = _fe.make_sim(2)
    runners = _runners(sim_cls, 2, (24, 12), geo='EqualSubdomainsGeometry2D', subdomains=2, conn_axis='y')
    group = LocalGroup(runners)
    for r in runners:
        r.prepare()
        assert r._startup_pending and 'SetInitialConditions' not in r.backend.launched
    group._startup_fields()
    log = runners[0].backend.launched          # (the group's queue performs every runner's entries through this backend)
    assert log.index('CollectSparseData') < log.index('DistributeSparseData') < log.index('SetInitialConditions')
    for r in runners:
        assert not r._startup_pending and 'SetInitialConditions' in r.backend.launched
        assert np.all(np.isfinite(r._sim.phi))
