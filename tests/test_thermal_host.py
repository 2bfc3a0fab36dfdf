"""Thermal flows, host layer: LBThermalFluidSim describes an ordinary accel_field module, ThermalSubdomainRunner puts the init
launch behind SetInitialConditions and the thermal launch behind every step's program, always with the full-output sweep;
what is not served is refused by name; the populations and the field travel with checkpoints; the example loads and runs.
Through a recording backend (tests/_thermal_backend.py): no GPU."""
import os

import numpy as np
import pytest

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish_amd import geo as geo_mod
from sailfish_amd import thermal
from sailfish_amd.lb_thermal import LBThermalFluidSim
from sailfish_amd.node_type import DynamicValue, NTFullBBWall
from sailfish_amd.subdomain import Subdomain2D, Subdomain3D
from sailfish_amd.sym import S
from tests import _host, _thermal_backend
from tests.test_accf_host import runners_of

SIZE = (24, 12)
B, T_REF, KAPPA = (0.0, 1e-3), 0.5, 0.1


def layer_sim(dim=2, buoyancy=B, force=(1e-5, 0.0), walls=True, pinned=False):
    base = Subdomain2D if dim == 2 else Subdomain3D

    class Layer(base):
        def boundary_conditions(self, *h):
            if walls:
                self.set_node((h[1] == 0) | (h[1] == self.gy - 1), NTFullBBWall)

        def initial_conditions(self, sim, *h):
            sim.rho[:] = 1.0
            sim.T[:] = 0.5 + 0.01 * h[0]
            if walls or pinned:
                sim.wall_temperature[h[1] == 0] = 1.0
                sim.wall_temperature[h[1] == self.gy - 1] = 0.0

    class Sim(LBThermalFluidSim):
        subdomain = Layer

        def __init__(self, config):
            super(Sim, self).__init__(config)
            self.set_buoyancy(tuple(buoyancy) + (0.0,) * (dim - len(buoyancy)), t_ref=T_REF)
            if force is not None:
                self.add_body_force(tuple(force) + (0.0,) * (dim - len(force)))

    return Sim


def cfg_of(size=SIZE, **over):
    cfg = dict(lat_nx=size[0], lat_ny=size[1], periodic_x=True, access_pattern='AB', precision='single', model='bgk', visc=0.05,
               thermal_diffusivity=KAPPA)
    if len(size) == 3:
        cfg.update(lat_nz=size[2], periodic_z=True)
    cfg.update(over)
    return cfg


def run(steps, sim=None, **over):
    from sailfish_amd.controller import LBSimulationController
    del _thermal_backend.LOG[:]
    cfg = cfg_of(max_iters=steps, quiet=True, perf_stats_every=0, gpus=[0], backends='tests._thermal_backend', output='', **over)
    ctrl = LBSimulationController(sim or layer_sim(), geo_mod.LBGeometry2D, default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    return ctrl, list(_thermal_backend.LOG)


def test_sim_describes_an_accel_field_module():
    _, (r,) = runners_of(layer_sim(), 2, 'LBGeometry2D', cfg_of(precision='double'))
    sim = r._sim
    assert isinstance(sim, LBThermalFluidSim) and sim.has_accel_field and sailfish.lb_thermal.LBThermalFluidSim is LBThermalFluidSim
    assert type(r).__name__ == 'ThermalSubdomainRunner'
    d = r._module_desc()
    assert d.accel_field == 1 and d.has_force == 1 and list(d.accel) == [1e-5, 0.0, 0.0]
    assert not r.accel_field_host().any()                    # the field starts from zero
    assert [f.name for f in sim.fields()] == ['rho', 'v', 'T', 'wall_temperature']
    assert sim.buoyancy == [0.0, 1e-3] and sim.t_ref == 0.5
    # the subdomain's initial_conditions wrote both fields; wall_temperature is NaN where nothing was set
    assert np.array_equal(sim.T[3], (0.5 + 0.01 * np.arange(SIZE[0])).astype(np.float64))
    assert (sim.wall_temperature[0] == 1.0).all() and (sim.wall_temperature[-1] == 0.0).all()
    assert np.isnan(sim.wall_temperature[1:-1]).all()
    with pytest.raises(ValueError, match='2 components'):
        sim.set_buoyancy((0.0, 1e-3, 0.0))


def test_options_and_tau():
    _, (r,) = runners_of(layer_sim(), 2, 'LBGeometry2D', cfg_of())
    assert r.config.thermal_diffusivity == KAPPA and r._sim.tau_T == 0.5 + 3.0 * KAPPA
    _, (r3,) = runners_of(layer_sim(3), 3, 'LBGeometry3D', cfg_of((10, 6, 5), thermal_diffusivity=0.05))
    assert r3._sim.tau_T == 0.5 + 4.0 * 0.05 and thermal.tau_of(0.05, 3) == 0.7
    assert thermal.Q == {2: 5, 3: 7}
    _, (d,) = runners_of(layer_sim(), 2, 'LBGeometry2D', dict((k, v) for k, v in cfg_of().items() if k != 'thermal_diffusivity'))
    assert d.config.thermal_diffusivity == 1.0 / 6.0 and d._sim.tau_T == 1.0         # the option's default
    for bad in (0.0, -0.1):
        _, (rb,) = runners_of(layer_sim(), 2, 'LBGeometry2D', cfg_of(thermal_diffusivity=bad))
        with pytest.raises(ValueError, match='--thermal_diffusivity must be > 0'):
            rb._module_desc()


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('plans', [True, False])
def test_call_sequence_of_a_step(pattern, plans):
    ctrl, log = run(6, access_pattern=pattern, hip_step_plans=plans)
    (r,) = ctrl.runners
    t = r._thermal
    kinds = [e[0] for e in log]
    assert log[0] == ('build', 1) and kinds.count('set_accel_field') == 1 and kinds.count('thermal_init') == 1
    init_at = kinds.index('thermal_init')
    inits = [i for i, e in enumerate(log) if e[0] == 'run' and e[1] == 'SetInitialConditions']
    assert inits and max(inits) < init_at                                   # behind the flow's SetInitialConditions
    assert kinds.index('set_accel_field') < init_at
    steps = [e for e in log[init_at + 1:] if e[0] == 'thermal_step' or (e[0] == 'run' and e[1] == 'CollideAndPropagate')]
    assert [e[0] for e in steps] == ['run', 'thermal_step'] * 6             # the thermal launch follows every sweep
    gmap, v = r.gpu_geo_map(), tuple(r.gpu_field(r._sim.v))
    params = (float(np.float32(1.0 / (0.5 + 3.0 * KAPPA))), T_REF, B, (True, False))
    init = log[init_at]
    assert init[1:] == (params, gmap, r.gpu_field(r._sim.T), v, t.gpu_g[0], r._calc_stream)
    for n, (sweep, back) in enumerate(zip(steps[0::2], steps[1::2])):
        assert sweep[2] & 1, 'the sweep stores rho and v at every step'
        assert sweep[3] is r._calc_stream
        assert back[1:] == (params, gmap, t.gpu_g[n & 1], t.gpu_g[1 - (n & 1)], v, r.gpu_field(r._sim.wall_temperature),
                            r.gpu_field(r._sim.T), r._calc_stream)
    assert t.gpu_g[0] != t.gpu_g[1] and t.host[0].shape == (5,) + tuple(r._physical_size) and t.host[0].dtype == np.float32
    assert r.fast_forward() == 0 and r._resident_setup() is None


def test_fluid_only_box_passes_no_map():
    ctrl, log = run(2, sim=layer_sim(walls=False), periodic_y=True)
    (r,) = ctrl.runners
    assert int(r._desc.fluid_only) == 1
    calls = [e for e in log if e[0] in ('thermal_init', 'thermal_step')]
    assert len(calls) == 3 and all(e[2] == 0 for e in calls) and calls[0][1][3] == (True, True)


def test_fixed_temperature_in_a_fluid_only_box_is_refused():
    """Without a node map the kernels never read a wet node's own wall_temperature: a finite entry is refused, not ignored."""
    with pytest.raises(ValueError, match='wall_temperature is finite at 48 nodes'):
        run(2, sim=layer_sim(walls=False, pinned=True), periodic_y=True)
    assert 'thermal_init' not in [e[0] for e in _thermal_backend.LOG]


def test_wall_temperature_is_not_an_output_field():
    ctrl, _ = run(2)
    (r,) = ctrl.runners
    assert [f.name for f in r._sim.fields() if not f.output] == ['wall_temperature']
    assert 'wall_temperature' not in r._output._scalar_fields and 'T' in r._output._scalar_fields
    assert r.gpu_field(r._sim.wall_temperature)                                # on the device all the same


def test_checkpoint_round_trip_of_the_populations_and_the_field(tmp_path):
    straight, _ = run(10)
    ck = str(tmp_path / 'ck')
    run(7, checkpoint_file=ck, final_checkpoint=True)
    cp = [f for f in os.listdir(str(tmp_path)) if f.endswith('.cpoint.npz')]
    assert len(cp) == 1
    restored, log = run(10, restore_from=os.path.join(str(tmp_path), cp[0][:-len('.0.cpoint.npz')]))
    backs = [e for e in log if e[0] == 'thermal_step']
    t = restored.runners[0]._thermal
    assert len(backs) == 3 and backs[0][3:5] == (t.gpu_g[1], t.gpu_g[0])          # step 7 reads copy 1: the parity came back
    step = np.float32(_thermal_backend.STEP)
    for ctrl in (straight, restored):
        r = ctrl.runners[0]
        g = r.thermal_populations()
        assert r._sim.iteration == 10 and (g == g.flat[0]).all() and g.flat[0] == 10 * step
        r.backend.from_buf(r._gpu_accel_field)
        assert (r._host_accel_field == 10 * step).all()
    state = straight.runners[0]._sim.get_state()
    assert 'thermal_g' not in state                                           # carried only once a checkpoint fetched it


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_more_than_one_subdomain_is_refused():
    with pytest.raises(NotImplementedError, match='more than one subdomain'):
        runners_of(layer_sim(force=None), 2, 'EqualSubdomainsGeometry2D', cfg_of(subdomains=2, conn_axis='x'))


def test_position_dependent_force_with_buoyancy_is_refused():
    sim = layer_sim(force=None)(_host.make_config(2, hip_accel_field=True, **cfg_of()))
    with pytest.raises(NotImplementedError, match='both would own the acceleration field'):
        sim.add_body_force(DynamicValue(1e-5 * S.gx, 0.0))
    from sympy import sin
    sim.add_body_force(DynamicValue(1e-5 * sin(S.time), 0.0))            # uniform forces are fine, time-dependent too
    sim.add_body_force((1e-5, 0.0))
    assert sim.time_dependent_force


@pytest.mark.parametrize('cfg,word', [
    (dict(grid='D3Q15'), 'D3Q15'), (dict(grid='D3Q27'), 'D3Q27'), (dict(model='elbm'), '--model=elbm'),
    (dict(regularized=True), '--regularized'), (dict(subgrid='les-smagorinsky'), '--subgrid'),
    (dict(minimize_roundoff=True), '--minimize_roundoff'), (dict(node_addressing='indirect'), '--node_addressing=indirect')],
    ids=lambda v: v if isinstance(v, str) else '')
def test_what_the_field_refuses_is_refused_by_name(cfg, word):
    base = cfg_of((10, 6, 5), periodic_y=True, precision='double')
    _, (r,) = runners_of(layer_sim(3, walls=False), 3, 'LBGeometry3D', dict(base, **cfg))
    with pytest.raises(NotImplementedError) as e:
        r._module_desc()
    assert word in str(e.value)


def test_tms_walls_are_refused():
    from sailfish_amd.node_type import NTWallTMS

    class Tms(Subdomain2D):
        def boundary_conditions(self, hx, hy):
            self.set_node((hy == 0) | (hy == self.gy - 1), NTWallTMS)

        def initial_conditions(self, sim, hx, hy):
            sim.rho[:] = 1.0

    class Sim(LBThermalFluidSim):
        subdomain = Tms

    _, (r,) = runners_of(Sim, 2, 'LBGeometry2D', cfg_of())
    with pytest.raises(NotImplementedError, match='NTWallTMS'):
        r._module_desc()


def test_backend_without_thermal_calls_and_bad_arguments_are_refused():
    class NoThermal(object):
        name = 'plain'
    with pytest.raises(NotImplementedError, match='slf_thermal'):
        thermal.ThermalLattice(NoThermal(), None, np.float32, 2, (1, 6, 32), (True, False), 0.1, 0.0, (0.0, 1e-3))
    b = _thermal_backend.ThermalRecordingBackend()
    with pytest.raises(ValueError, match='diffusivity must be > 0'):
        thermal.ThermalLattice(b, None, np.float32, 2, (1, 6, 32), (True, False), 0.0, 0.0, (0.0, 1e-3))
    with pytest.raises(ValueError, match='2 components'):
        thermal.ThermalLattice(b, None, np.float32, 2, (1, 6, 32), (True, False), 0.1, 0.0, (0.0, 1e-3, 0.0))


# ---- the example ------------------------------------------------------------------------------------------------------------------

def test_rayleigh_benard_example_loads_and_runs_three_steps(capsys):
    from examples.rayleigh_benard_2d import RayleighBenardSimulation
    _, (r,) = runners_of(RayleighBenardSimulation, 2, 'LBGeometry2D', {})
    sim, cfg = r._sim, r.config
    assert (cfg.lat_nx, cfg.lat_ny, cfg.visc, cfg.Ra, cfg.Pr, cfg.periodic_x) == (128, 66, 0.03, 5000.0, 1.0, True)
    assert cfg.thermal_diffusivity == 0.03 and sim.t_ref == 0.5
    assert sim.buoyancy[0] == 0.0 and abs(sim.buoyancy[1] - 5000.0 * 0.03 * 0.03 / 64.0 ** 3) < 1e-18
    assert r._module_desc().accel_field == 1
    assert (sim.wall_temperature[0] == 1.0).all() and (sim.wall_temperature[-1] == 0.0).all()
    assert abs(sim.T[1:-1].mean() - 0.5) < 1e-6 and np.ptp(sim.T[32]) > 1e-3       # conduction profile + the perturbation
    _, (p,) = runners_of(RayleighBenardSimulation, 2, 'LBGeometry2D', dict(Ra=2000.0, Pr=0.5, lat_ny=34))
    assert p.config.thermal_diffusivity == 0.06 and abs(p._sim.buoyancy[1] - 2000.0 * 0.03 * 0.06 / 32.0 ** 3) < 1e-18
    from sailfish_amd.controller import LBSimulationController
    del _thermal_backend.LOG[:]
    ctrl = LBSimulationController(RayleighBenardSimulation, geo_mod.LBGeometry2D,
                                  default_config=dict(lat_nx=32, lat_ny=18, max_iters=3, every=2, quiet=True, perf_stats_every=0,
                                                      gpus=[0], backends='tests._thermal_backend', output=''))
    ctrl.run(ignore_cmdline=True)
    assert [e[0] for e in _thermal_backend.LOG].count('thermal_step') == 3
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln and ln[0].isdigit()]
    assert lines and lines[0][0] == '2' and len(lines[0]) == 3                      # iteration, energy, Nusselt number
