"""Host side of the ternary Shan-Chen mixture (no GPU): the reference's import path, options, constants, the module
descriptor, kernel names and argument lists, body forces on lattice 2, and what is refused when a simulation is set up."""
import argparse
import ctypes

import pytest

from sailfish_amd import hipabi, lb_base, sym
from sailfish_amd import node_type as nt
from tests import _host, _sc, _sc3
from tests.test_elbm_host import RecordingBackend


class LoggingBackend(RecordingBackend):
    """Records the names of the kernels that are launched, in order."""

    def __init__(self, *a, **kw):
        super(LoggingBackend, self).__init__(*a, **kw)
        self.launched = []

    def run_kernel(self, k, grid_size=None, stream=None):
        self.launched.append(k.name)


class FusedBackend(LoggingBackend):
    supports_fused_shan_chen = True


def _runners(sim_cls, dim, size, geo=None, backend=LoggingBackend, **kw):
    cfg = _sc3.config(dim, size, **kw)
    return _host.build_runners(sim_cls, dim, geo, cfg, backend_factory=backend)[2]


def test_the_reference_import_path():
    from sailfish.lb_ternary import LBTernaryFluidBase, LBTernaryFluidShanChen
    from sailfish_amd import lb_ternary, subdomain_runner
    assert LBTernaryFluidShanChen is lb_ternary.LBTernaryFluidShanChen
    assert issubclass(LBTernaryFluidShanChen, LBTernaryFluidBase) and issubclass(LBTernaryFluidShanChen, lb_base.LBForcedSim)
    assert LBTernaryFluidShanChen.subdomain_runner is subdomain_runner.NNSubdomainRunner
    assert LBTernaryFluidShanChen.nonlocality == 1


def test_options_defaults_fields_and_constants():
    from sailfish.lb_ternary import LBTernaryFluidShanChen
    p = argparse.ArgumentParser()
    for base in LBTernaryFluidShanChen.mro():
        if 'add_options' in base.__dict__ and base is not lb_base.LBSim:
            base.add_options(p, 2)
    o = p.parse_args([])
    # reference lb_ternary.py:28-32, :195-211
    assert (o.tau_phi, o.tau_theta, o.visc, o.sc_potential) == (1.0, 1.0, 1.0, 'linear')
    assert (o.G11, o.G12, o.G13, o.G22, o.G23, o.G33) == (0.0,) * 6
    assert p.parse_args(['--sc_potential=classic']).sc_potential == 'classic'
    with pytest.raises(SystemExit):
        p.parse_args(['--sc_potential=cubic'])
    assert [(type(f).__name__, f.name, f.need_nn) for f in LBTernaryFluidShanChen.fields()] == [
        ('ScalarField', 'rho', True), ('ScalarField', 'phi', True), ('ScalarField', 'theta', True),
        ('VectorField', 'v', False)]
    o = p.parse_args(['--G11=1', '--G12=2', '--G13=3', '--G22=4', '--G23=5', '--G33=6'])
    o.grid = 'D2Q9'
    sim = LBTernaryFluidShanChen(o)
    assert len(sim.grids) == 3
    c = sim.constants()
    assert c == dict(G11=1.0, G12=2.0, G13=3.0, G21=2.0, G22=4.0, G23=5.0, G31=3.0, G32=5.0, G33=6.0)
    assert list(sim._force_couplings.items()) == [((k, j), 'G%d%d' % (k + 1, j + 1)) for k in range(3) for j in range(3)]


@pytest.mark.parametrize('dim,size', [(2, (24, 12)), (3, (20, 12, 10))])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('fused', [False, True], ids=['three kernels', 'fused'])
def test_descriptor_and_kernel_argument_lists(dim, size, pattern, fused, monkeypatch):
    monkeypatch.delenv('SLF_SC_FUSED', raising=False)
    a0, a2 = [1e-5, 0.0, 2e-5][:dim], [0.0, -3e-5, 4e-5][:dim]
    sim_cls, _ = _sc3.make_sim(dim, walls=True, forces={0: a0, 2: a2})
    r = _runners(sim_cls, dim, size, pattern=pattern, potential='classic', force='edm',
                 backend=FusedBackend if fused else LoggingBackend)[0]
    r.prepare()
    d = r.backend.desc
    P = _sc3.PARAMS
    assert d.struct_size == ctypes.sizeof(hipabi.SlfModuleDesc)
    assert d.simtype == hipabi.SLF_SIM_SHAN_CHEN_TERNARY == 4 and d.model == hipabi.SLF_BGK
    assert (d.tau, d.tau_phi, d.tau_theta) == (sym.relaxation_time(P['visc']), P['tau_phi'], P['tau_theta'])
    assert list(d.sc3_G) == [P['G11'], P['G12'], P['G13'], P['G12'], P['G22'], P['G23'], P['G13'], P['G23'], P['G33']]
    assert d.sc_potential == 1 and d.force_implementation == hipabi.SLF_FORCE_EDM
    assert d.has_force == 1 and list(d.accel)[:dim] == a0 and list(d.accel1) == [0.0] * 3 and list(d.accel2)[:dim] == a2
    assert d.fluid_only == 0 and d.node_addressing == hipabi.SLF_ADDR_DIRECT
    sim = r._sim
    fields = [r.gpu_field(sim.rho), r.gpu_field(sim.phi), r.gpu_field(sim.theta)]
    v = r.gpu_field(sim.v)
    gmap = r.gpu_geo_map()
    for kernels in (r._kernels_none, r._kernels_full):
        assert len(kernels) == 2
        for parity, (macro, sweeps) in enumerate(kernels):
            src = 0 if (pattern == 'AA' or parity == 0) else 1
            dst = 0 if pattern == 'AA' else 1 - src
            options = 3 if kernels is r._kernels_full else 2
            assert macro.name == 'ShanChenPrepareMacroFields' and macro.fmt == 'P' * (7 + dim) + 'i'
            assert macro.args == [gmap] + [r.gpu_dist(k, src) for k in range(3)] + fields + v + [options]
            if fused:
                assert [k.name for k in sweeps] == ['ShanChenCollideAndPropagateFused']
                assert sweeps[0].fmt == 'P' * (10 + dim) + 'i'
                pairs = [x for k in range(3) for x in (r.gpu_dist(k, src), r.gpu_dist(k, dst))]
                assert sweeps[0].args == [gmap] + pairs + fields + v + [options]
            else:
                assert [k.name for k in sweeps] == ['ShanChenCollideAndPropagate%d' % k for k in range(3)]
                for k, kern in enumerate(sweeps):
                    assert kern.fmt == 'P' * (6 + dim) + 'i'
                    assert kern.args == [gmap, r.gpu_dist(k, src), r.gpu_dist(k, dst)] + fields + v + [options]
    assert r.backend.launched.count('SetInitialConditions') == (2 if pattern == 'AB' else 1)
    assert len(set(r.gpu_dist(k, c) for k in range(3) for c in (0, 1))) == (6 if pattern == 'AB' else 3)


def test_the_switch_selects_the_three_kernels(monkeypatch):
    monkeypatch.setenv('SLF_SC_FUSED', '0')
    sim_cls, _ = _sc3.make_sim(2)
    r = _runners(sim_cls, 2, (24, 12), backend=FusedBackend)[0]
    r.prepare()
    assert [k.name for k in r._kernels_none[0][1]] == ['ShanChenCollideAndPropagate%d' % k for k in range(3)]


@pytest.mark.parametrize('fused', [True, False], ids=['in-sweep wrap', 'ghost-layer kernels'])
def test_periodic_boundary_kernels_cover_three_lattices_and_three_fields(fused):
    sim_cls, _ = _sc3.make_sim(3)
    r = _runners(sim_cls, 3, (20, 12, 10), fused=fused, pattern='AA')[0]
    r.prepare()
    pbc = r._pbc_kernels
    sim = r._sim
    fields = [r.gpu_field(sim.rho), r.gpu_field(sim.phi), r.gpu_field(sim.theta)]
    for axis in range(3):
        assert [k.name for k in pbc.distributions[0][axis]] == ['ApplyPeriodicBoundaryConditions'] * 3
        assert [k.name for k in pbc.distributions[1][axis]] == ['ApplyPeriodicBoundaryConditionsWithSwap'] * 3
        assert [k.args for k in pbc.distributions[1][axis]] == [[r.gpu_dist(k, 0), axis] for k in range(3)]
        for copy in (0, 1):
            assert [k.args for k in pbc.macro[copy][axis]] == [[f, axis] for f in fields]
    assert list(r._pbc_axes) == ([] if fused else [0, 1, 2])


def test_halo_carries_three_lattices_and_three_fields():
    sim_cls, _ = _sc3.make_sim(3)
    for axis in 'xyz':
        runners = _runners(sim_cls, 3, (20, 12, 10), geo='EqualSubdomainsGeometry3D', subdomains=2, conn_axis=axis)
        for r in runners:
            r.prepare()
            assert r._nnx is None                                   # no x-face planes: ghost columns and index lists
            assert r._links and r._macro_links
            for link in r._links.values():
                assert len(link.packs[0]) == 3 and len(link.unpacks[0]) == 3
            for link in r._macro_links.values():
                assert len(link.packs[0]) == 3 and len(link.unpacks[0]) == 3


def test_body_force_on_lattice_two():
    from sailfish.lb_ternary import LBTernaryFluidShanChen
    sim_cls, _ = _sc3.make_sim(2, forces={2: (1e-5, 2e-5)})
    r = _runners(sim_cls, 2, (24, 12))[0]
    r.prepare()
    d = r.backend.desc
    assert list(d.accel2) == [1e-5, 2e-5, 0.0] and d.has_force == 0 and list(d.accel1) == [0.0] * 3
    assert issubclass(sim_cls, LBTernaryFluidShanChen)
    # lattice 2 exists in ternary models only
    binary, _ = _sc.make_sim(2)

    class Cfg(object):
        grid = 'D2Q9'
    with pytest.raises(NotImplementedError, match='lattices 0 and 1'):
        binary(Cfg()).add_body_force((1e-5, 0.0), grid=2)
    with pytest.raises(NotImplementedError, match='lattices 0 and 1'):
        sim_cls(Cfg()).add_body_force((1e-5, 0.0), grid=3)


class _HalfWalls(_sc3.Subdomain2D):
    def boundary_conditions(self, hx, hy):
        self.set_node((hy == 0) | (hy == self.gy - 1), nt.NTHalfBBWall)

    def initial_conditions(self, sim, hx, hy):
        sim.rho[:] = 1.0
        sim.phi[:] = 1.0
        sim.theta[:] = 1.0


class _PressureWalls(_HalfWalls):
    def boundary_conditions(self, hx, hy):
        self.set_node(hy == 0, nt.NTEquilibriumDensity(1.0))


def _sim_with(subdomain_cls, init=None):
    from sailfish.lb_ternary import LBTernaryFluidShanChen

    class Sim(LBTernaryFluidShanChen):
        subdomain = subdomain_cls

        def __init__(self, config):
            super(Sim, self).__init__(config)
            if init:
                init(self)
    return Sim


PLAIN = _sc3.make_sim(2)[0]
REFUSALS = [
    ('indirect', PLAIN, dict(node_addressing='indirect'), 'node_addressing=indirect'),
    ('mrt', PLAIN, dict(model='mrt'), 'model=mrt'),
    ('elbm', PLAIN, dict(model='elbm'), 'model=elbm'),
    ('half-way walls', _sim_with(_HalfWalls), dict(periodic_y=False), 'NTFullBBWall nodes only'),
    ('other boundary types', _sim_with(_PressureWalls), dict(periodic_y=False), 'NTFullBBWall nodes only'),
    ('minimize_roundoff', PLAIN, dict(minimize_roundoff=True), 'minimize_roundoff'),
]


@pytest.mark.parametrize('name,sim_cls,over,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_when_the_simulation_is_set_up(name, sim_cls, over, message):
    with pytest.raises(NotImplementedError, match=message):
        r = _runners(sim_cls, 2, (24, 12), **over)[0]
        r.prepare()


def test_force_objects_are_refused():
    def add(sim):
        sim.add_force_oject(lb_base.ForceObject((3, 3), (5, 5)))
    with pytest.raises(NotImplementedError, match='force objects: single-fluid'):
        _runners(_sim_with(PLAIN.subdomain, add), 2, (24, 12))[0].prepare()


def test_the_descriptor_mirror_keeps_the_entropic_fields_last():
    names = [f[0] for f in hipabi.SlfModuleDesc._fields_]
    assert names[-3:] == ['entropic_equilibrium', 'entropy_tolerance', 'alpha_tolerance']
    assert names.index('fe_zero_grad_rim') < names.index('tau_theta') < names.index('sc3_G') < names.index('accel2') < \
        names.index('entropic_equilibrium')
