"""Immersed boundary markers, host layer: LBIBMFluidSim describes an ordinary accel_field module, IBMSubdomainRunner uploads
the markers and puts spread / gather in front of and clear-and-advect behind every step's program, always with the
full-output sweep; what is not served is refused by name; positions travel with checkpoints; the reference's own
ibm_cylinder.py loads.  Through a recording backend (tests/_ibm_backend.py): no GPU."""
import importlib.util
import os

import numpy as np
import pytest

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish_amd import geo as geo_mod
from sailfish_amd import hipabi
from sailfish_amd.lb_single import LBIBMFluidSim, Particle
from sailfish_amd.node_type import DynamicValue
from sailfish_amd.sym import S
from tests import _bind, _host, _ibm, _ibm_backend
from tests.test_accf_host import runners_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sailfish_amd', 'csrc')
HAVE_REF = os.path.isdir('/root/reference/examples')
SIZE = (24, 12)


def markers(n=5):
    pos = np.array(_ibm.ring((11.5, 5.5), 3.0, n))
    return pos, pos + 0.25, np.full(n, 0.01)


def run(steps, sim=None, **over):
    from sailfish_amd.controller import LBSimulationController
    del _ibm_backend.LOG[:]
    pos, ref, k = markers()
    sim = sim or _ibm.channel_sim(2, pos, ref, k, (1e-5, 0.0))
    cfg = _ibm.channel_cfg(SIZE, max_iters=steps, quiet=True, perf_stats_every=0, gpus=[0], backends='tests._ibm_backend',
                           output='', **over)
    ctrl = LBSimulationController(sim, geo_mod.LBGeometry2D, default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    return ctrl, list(_ibm_backend.LOG)


def test_sim_describes_an_accel_field_module():
    pos, ref, k = markers()
    _, (r,) = runners_of(_ibm.channel_sim(2, pos, ref, k, (1e-5, 0.0)), 2, 'LBGeometry2D',
                         _ibm.channel_cfg(SIZE, precision='double'))
    sim = r._sim
    assert isinstance(sim, LBIBMFluidSim) and sim.has_accel_field and sim.num_particles == 5
    assert type(r).__name__ == 'IBMSubdomainRunner'
    d = r._module_desc()
    assert d.accel_field == 1 and d.has_force == 1 and list(d.accel) == [1e-5, 0.0, 0.0]
    assert not r.accel_field_host().any()                    # the field starts from zero
    assert [f.name for f in sim.fields()] == ['rho', 'v', 'force'] and len(sim.force) == 2
    p = Particle((1.5, 2.5))
    assert p.ref_position == (1.5, 2.5) and p.stiffness == 1.0 and p.mass == 1.0
    with pytest.raises(ValueError):
        sim.add_particle(Particle((1.0, 2.0, 3.0)))


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('plans', [True, False])
def test_call_sequence_of_a_step(pattern, plans):
    ctrl, log = run(6, access_pattern=pattern, hip_step_plans=plans)
    (r,) = ctrl.runners
    m = r._markers
    kinds = [e[0] for e in log]
    assert log[0] == ('build', 1) and kinds.count('set_accel_field') == 1
    assert not log[kinds.index('set_accel_field')][2].any()                    # a zero field
    assert kinds.index('set_accel_field') < kinds.index('ibm_spread')
    steps = [e for e in log if e[0].startswith('ibm_') or (e[0] == 'run' and e[1] == 'CollideAndPropagate')]
    assert [e[0] for e in steps] == ['ibm_spread', 'ibm_gather', 'run', 'ibm_clear_and_advect'] * 6
    for e in steps:
        if e[0] == 'run':
            assert e[2] & 1, 'the sweep stores rho and v at every step'
            assert e[3] is r._calc_stream
        else:
            assert e[1] == 5 and e[2] == (0, 0) and e[-1] is r._calc_stream
    spread, gather, _, back = steps[:4]
    assert spread[3:7] == (m.gpu_position, m.gpu_ref_position, m.gpu_stiffness, m.gpu_acc)
    assert gather[3:5] == (m.gpu_position, m.gpu_acc)
    assert back[3:8] == (m.gpu_position, m.gpu_acc, r.gpu_geo_map(), tuple(r.gpu_field(r._sim.v)), m.gpu_outside)
    assert m.acc.dtype == np.int64 and m.acc.size == 2 * np.prod(r._physical_size) and not m.acc.any()
    # what was uploaded: [dim, n] in the run's precision
    pos, ref, k = markers()
    assert np.array_equal(m.ref_position, ref.T.astype(np.float32)) and np.array_equal(m.stiffness, k.astype(np.float32))
    # positions: copied back on request and whenever the fields are (the last step syncs them)
    want = (pos.astype(np.float32) + np.float32(6 * _ibm_backend.STEP))
    assert np.array_equal(r.particle_positions(), want) and np.array_equal(r._sim.particle_positions, want)
    assert r.fast_forward() == 0 and r._resident_setup() is None


def test_no_markers_is_the_plain_field_run_through_the_full_output_kernels():
    ctrl, log = run(4, sim=_ibm.channel_sim(2, [], [], [], (1e-5, 0.0)))
    (r,) = ctrl.runners
    assert r._markers is None and r.ibm_outside == 0 and r.particle_positions().shape == (0, 2)
    assert not [e for e in log if e[0].startswith('ibm_')]
    sweeps = [e for e in log if e[0] == 'run' and e[1] == 'CollideAndPropagate']
    assert len(sweeps) == 4 and all(e[2] & 1 for e in sweeps)


def test_checkpoint_round_trip_of_the_positions(tmp_path):
    straight, _ = run(10)
    ck = str(tmp_path / 'ck')
    run(7, checkpoint_file=ck, final_checkpoint=True)
    cp = [f for f in os.listdir(str(tmp_path)) if f.endswith('.cpoint.npz')]
    assert len(cp) == 1
    restored, log = run(10, restore_from=os.path.join(str(tmp_path), cp[0][:-len('.0.cpoint.npz')]))
    assert [e[0] for e in log].count('ibm_spread') == 3
    pos = markers()[0].astype(np.float32)
    for ctrl in (straight, restored):
        assert np.array_equal(ctrl.runners[0].particle_positions(), pos + np.float32(10 * _ibm_backend.STEP))
        assert np.array_equal(ctrl.runners[0]._sim.particle_positions, pos + np.float32(10 * _ibm_backend.STEP))


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_more_than_one_subdomain_is_refused():
    pos, ref, k = markers()
    with pytest.raises(NotImplementedError, match='more than one subdomain'):
        runners_of(_ibm.channel_sim(2, pos, ref, k, None), 2, 'EqualSubdomainsGeometry2D',
                   _ibm.channel_cfg(SIZE, subdomains=2, conn_axis='x'))


def test_position_dependent_force_with_markers_is_refused():
    sim = _ibm.channel_sim(2, [], [], [], None)(_host.make_config(2, hip_accel_field=True, **_ibm.channel_cfg(SIZE)))
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
    pos = [(4.5, 3.5, 2.5)]
    sim = _ibm.channel_sim(3, pos, pos, [0.01], (1e-5, 0.0, 0.0), walls=False)
    base = _ibm.channel_cfg((10, 6, 5), periodic_y=True, precision='double')
    _, (r,) = runners_of(sim, 3, 'LBGeometry3D', dict(base, **cfg))
    with pytest.raises(NotImplementedError) as e:
        r._module_desc()
    assert word in str(e.value)


def test_tms_walls_are_refused():
    from sailfish_amd.node_type import NTWallTMS
    from sailfish_amd.subdomain import Subdomain2D

    class Tms(Subdomain2D):
        def boundary_conditions(self, hx, hy):
            self.set_node((hy == 0) | (hy == self.gy - 1), NTWallTMS)

        def initial_conditions(self, sim, hx, hy):
            sim.rho[:] = 1.0

    class Sim(LBIBMFluidSim):
        subdomain = Tms

    _, (r,) = runners_of(Sim, 2, 'LBGeometry2D', _ibm.channel_cfg(SIZE))
    with pytest.raises(NotImplementedError, match='NTWallTMS'):
        r._module_desc()


def test_backend_without_marker_calls_is_refused():
    from sailfish_amd import ibm

    class NoIbm(object):
        name = 'plain'
    with pytest.raises(NotImplementedError, match='slf_ibm'):
        ibm.Markers(NoIbm(), None, np.float32, 2, (0, 0), [[1.0, 1.0]], [[1.0, 1.0]], [0.1])


# ---- the examples ----------------------------------------------------------------------------------------------------------------

def check_cylinder(sim_cls):
    _, (r,) = runners_of(sim_cls, 2, 'LBGeometry2D', {})
    sim, cfg = r._sim, r.config
    assert (cfg.lat_nx, cfg.lat_ny, cfg.visc) == (512, 128, 0.01)
    assert sim.num_particles == 50 and r._module_desc().accel_field == 1
    pos = np.array([p.position for p in sim._particles])
    assert np.allclose(np.hypot(pos[:, 0] - 128.0, pos[:, 1] - 64.0), 10.0, rtol=1e-14)
    assert all(p.stiffness == 0.01 and p.ref_position == p.position for p in sim._particles)
    force = sim.body_force_at(0)
    assert np.allclose(force, [150 / 20.0 * 0.01 / 400.0 * 8 * 0.01, 0.0])
    return sim


def test_ibm_cylinder_example_loads():
    from examples.ibm_cylinder import CylinderSimulation
    sim = check_cylinder(CylinderSimulation)
    sim.iteration = 20
    sim.vx[...] = 0.0
    sim.vy[...] = 0.0
    sim.after_step(None)                                                # integer indices: no IndexError


@pytest.mark.skipif(not HAVE_REF, reason='/root/reference not available on this machine')
def test_reference_ibm_cylinder_loads_unchanged():
    spec = importlib.util.spec_from_file_location('refexample_ibm_cylinder', '/root/reference/examples/ibm_cylinder.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    check_cylinder(mod.CylinderSimulation)


# ---- the argument checks of the C ABI, stand-alone ----------------------------------------------------------------------------

def test_bind_program_walks_the_argument_checks(tmp_path):
    """tests/ibm_bind_main.cpp against csrc/slf_bind.h, built with the address and undefined-behaviour sanitizers and run as a
    child process: nothing is loaded into Python."""
    done = _bind.run('ibm_bind_main.cpp', tmp_path)
    assert done.returncode == 0, done.stderr[-4000:]
    rows = {ln.split('\t')[0]: ln.split('\t') for ln in done.stdout.splitlines()}
    OK, INVALID, UNSUPPORTED = 0, 1, 3
    for subject in ('served-d2q9', 'served-d3q19-f64'):
        assert int(rows[subject][1]) == OK, rows[subject]
    want = {'no-accel-field': (INVALID, 'accel_field'), 'field-not-set': (INVALID, 'slf_module_set_accel_field'),
            'zero-markers': (INVALID, 'positive'), 'negative-markers': (INVALID, 'positive'),
            'too-many-markers': (INVALID, '2^24'), 'null-origin': (INVALID, 'origin is NULL'),
            'origin-out-of-range': (INVALID, '2^30'), 'null-pos': (INVALID, 'pos is NULL'),
            'null-acc': (INVALID, 'acc is NULL'), 'd3q15': (UNSUPPORTED, 'D3Q15'), 'd3q27': (UNSUPPORTED, 'D3Q15 / D3Q27')}
    assert set(want) | {'served-d2q9', 'served-d3q19-f64'} == set(rows)
    for subject, (code, word) in want.items():
        assert int(rows[subject][1]) == code and word in rows[subject][2], rows[subject]
        assert rows[subject][2].startswith('slf_ibm_test: ')
    assert hipabi.SIGNATURES['slf_ibm_spread'] and hipabi.SIGNATURES['slf_ibm_gather'] and \
        hipabi.SIGNATURES['slf_ibm_clear_and_advect'] and hipabi.SIGNATURES['slf_ibm_workspace_bytes']
