"""GPU tests of the full stack: examples -> LBSimulationController -> SubdomainRunner(s) ->
backend_hip -> libsailfish_hip.so, compared with the oracle twin (tests/_oracle_group.py) that uses
the same geometry, descriptors and halo lists.  Includes the reference's 1-vs-N subdomain
equivalence (regtest/subdomains/*.py), here with all subdomains on the one GPU of the test box, its
AB == AA check (tests/gpu/access_pattern.sh) and its checkpoint round trip (tests/gpu/checkpoint.sh).
"""
import os

import numpy as np
import pytest

from tests import _host
from tests._oracle_group import OracleGroup

pytestmark = pytest.mark.gpu

GEO = {2: 'EqualSubdomainsGeometry2D', 3: 'EqualSubdomainsGeometry3D'}


def run_gpu(module, sim, dim, cfg, steps, extra=None):
    """module: the name of an example (with `sim` its class name), or a simulation class itself."""
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    sim_cls = module if isinstance(module, type) else _host.load_sim_class(module, sim)
    defaults = dict(cfg)
    defaults.update(max_iters=steps, quiet=True, perf_stats_every=0)
    if extra:
        defaults.update(extra)
    ctrl = LBSimulationController(sim_cls, getattr(geo_mod, GEO[dim]), default_config=defaults)
    ctrl.run(ignore_cmdline=True)
    return ctrl


def merged_gpu(ctrl, what):
    r0 = ctrl.runners[0]
    gshape = tuple(reversed(r0._global_size))
    if what == 'dist':
        out = np.zeros((r0._sim.grid.Q,) + gshape, dtype=r0.float)
    else:
        out = np.zeros(gshape, dtype=r0.float)
    for r in ctrl.runners:
        sp = r._spec
        sl = tuple(slice(o, o + n) for o, n in zip(reversed(sp.location), reversed(sp.size)))
        if what == 'dist':
            d = r._debug_get_dist()
            out[(slice(None),) + sl] = d[(slice(None),) + tuple(sp._nonghost_slice)]
        elif what == 'rho':
            out[sl] = r._sim.rho
        else:
            out[sl] = r._sim.v[int(what[1])]
    return out


def check_against_oracle(module, sim, dim, cfg, steps, u_scale):
    ctrl = run_gpu(module, sim, dim, cfg, steps)
    og = OracleGroup(module if isinstance(module, type) else _host.load_sim_class(module, sim), dim, GEO[dim], cfg)
    og.run(steps, save_last=True)
    rho_g, rho_o = merged_gpu(ctrl, 'rho'), og.merged('rho')
    wet = np.isfinite(rho_o) & (rho_o != 0)
    assert np.max(np.abs(rho_g[wet] - rho_o[wet]) / np.abs(rho_o[wet])) < 1e-6
    for d in range(dim):
        a, b = merged_gpu(ctrl, 'v%d' % d), og.merged('v%d' % d)
        assert np.max(np.abs(a[wet] - b[wet])) / u_scale < 1e-6
    fg, fo = merged_gpu(ctrl, 'dist'), og.merged('dist')
    m = np.isfinite(fo)
    assert np.array_equal(np.isfinite(fg), m)
    assert np.max(np.abs(fg[m] - fo[m])) < 1e-7
    return ctrl, np.array_equal(fg[m], fo[m])


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('nsub,axis', [(1, 'x'), (3, 'x'), (2, 'y')])
def test_ldc_2d(pattern, nsub, axis):
    cfg = dict(lat_nx=66, lat_ny=40, visc=0.0254, access_pattern=pattern, subdomains=nsub, conn_axis=axis)
    check_against_oracle('ldc_2d', 'LDCSim', 2, cfg, 40, 0.1)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('nsub,axis,model', [(1, 'x', 'bgk'), (2, 'z', 'mrt'), (2, 'y', 'bgk'), (2, 'x', 'bgk')])
def test_ldc_3d(pattern, nsub, axis, model):
    cfg = dict(lat_nx=24, lat_ny=18, lat_nz=16, visc=0.03, model=model, access_pattern=pattern,
               subdomains=nsub, conn_axis=axis)
    check_against_oracle('ldc_3d', 'LDCSim', 3, cfg, 30, 0.05)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('wall,fused,nsub,axis', [('fullbb', True, 1, 'x'), ('halfbb', False, 1, 'x'),
                                                  ('halfbb', True, 2, 'y'), ('fullbb', False, 2, 'x')])
def test_poiseuille_force(pattern, wall, fused, nsub, axis):
    cfg = dict(lat_nx=24, lat_ny=40, visc=0.1, horizontal=False, stationary=False, drive='force', wall=wall,
               force_implementation='guo', access_pattern=pattern, hip_fused_periodic=fused,
               subdomains=nsub, conn_axis=axis)
    check_against_oracle('poiseuille', 'PoiseuilleSim', 2, cfg, 50, 0.02)


def test_poiseuille_pressure_mrt():
    cfg = dict(lat_nx=24, lat_ny=40, visc=0.1, horizontal=False, stationary=True, drive='pressure', wall='fullbb',
               force_implementation='guo', access_pattern='AB', model='mrt')
    check_against_oracle('poiseuille', 'PoiseuilleSim', 2, cfg, 50, 0.02)


@pytest.mark.parametrize('nsub,axis', [(1, 'z'), (2, 'z'), (2, 'x')])
def test_pipe_3d(nsub, axis):
    cfg = dict(lat_nx=18, lat_ny=18, lat_nz=16, visc=0.1, flow_direction='z', stationary=False, drive='force',
               force_implementation='guo', access_pattern='AA', subdomains=nsub, conn_axis=axis)
    check_against_oracle('poiseuille_3d', 'PoiseuilleSim', 3, cfg, 30, 0.02)


def test_poiseuille_converges_to_parabola():
    """Physics known answer (reference examples/poiseuille.py:73-83, regtest/poiseuille.py): the steady
    force-driven profile between half-way bounce-back walls is the parabola with u_max = max_v."""
    cfg = dict(lat_nx=8, lat_ny=34, visc=0.1, horizontal=True, stationary=True, drive='force', wall='halfbb',
               force_implementation='guo', access_pattern='AA')
    ctrl = run_gpu('poiseuille', 'PoiseuilleSim', 2, cfg, 3000)
    r = ctrl.runners[0]
    vx = r._sim.vx[:, 3]
    sub = r._subdomain
    hy = np.arange(34)
    ref = sub.velocity_profile(r.config, hy)
    err = np.max(np.abs(vx - ref)) / ref.max()
    assert err < 5e-3, err


def test_output_files_and_checkpoint_roundtrip(tmp_path):
    """103 steps + checkpoint, restore, continue to 200 == straight 200 (reference tests/gpu/checkpoint.sh),
    and the NPY output naming / masking (reference io.py:170-191, 53-59)."""
    base = dict(lat_nx=34, lat_ny=26, visc=0.02, access_pattern='AA')
    out = str(tmp_path / 'ldc')
    ctrl = run_gpu('ldc_2d', 'LDCSim', 2, base, 200, extra=dict(output=out, every=100))
    f200 = np.load(out + '.0.200.npz')
    assert set(f200.files) == {'rho', 'v'} and f200['v'].shape == (2, 26, 34)
    assert np.isnan(f200['rho'][0, 5])          # full-BB wall node is masked
    assert np.array_equal(f200['rho'][1:-1, 1:-1], ctrl.runners[0]._sim.rho[1:-1, 1:-1])
    ck = str(tmp_path / 'ck')
    run_gpu('ldc_2d', 'LDCSim', 2, base, 103, extra=dict(checkpoint_file=ck, final_checkpoint=True))
    cp = [f for f in os.listdir(str(tmp_path)) if f.startswith('ck') and f.endswith('.cpoint.npz')]
    assert len(cp) == 1
    restored = run_gpu('ldc_2d', 'LDCSim', 2, base, 200,
                       extra=dict(restore_from=os.path.join(str(tmp_path), cp[0][:-len('.0.cpoint.npz')])))
    assert restored.runners[0]._sim.iteration == 200
    # (the run with --output masked its non-fluid nodes with NaN; compare the wet interior)
    assert np.array_equal(restored.runners[0]._sim.rho[1:-1, 1:-1], ctrl.runners[0]._sim.rho[1:-1, 1:-1])
    assert np.array_equal(restored.runners[0]._debug_get_dist(), ctrl.runners[0]._debug_get_dist(), equal_nan=True)


def test_ldc_2d_re1000_matches_erturk(golden_dir):
    """Physics regression of BASELINE config 1 (examples/ldc_2d.py, D2Q9 BGK 256x256, Re = 1000,
    visc = 0.0254): steady centre-line velocities against Erturk et al. (reference regtest/ldc_2d.py,
    regtest/ldc_golden/vx2d, vy2d)."""
    n = 256
    cfg = dict(lat_nx=n, lat_ny=n, visc=(n - 2) * 0.1 / 1000.0, access_pattern='AA')
    ctrl = run_gpu('ldc_2d', 'LDCSim', 2, cfg, 160000)
    sim = ctrl.runners[0]._sim
    u_lid = 0.1
    # u along the vertical centre line, v along the horizontal centre line (mean of the two middle columns/rows)
    u_c = 0.5 * (sim.vx[:, n // 2] + sim.vx[:, n // 2 - 1]) / u_lid
    v_c = 0.5 * (sim.vy[n // 2, :] + sim.vy[n // 2 - 1, :]) / u_lid
    # the walls sit half-way between the wall node and the first fluid node (full-way bounce-back); the lid
    # is on the last row
    pos = (np.arange(n) - 0.5) / (n - 2)
    vy2d = np.loadtxt(os.path.join(golden_dir, 'ldc_golden', 'vy2d'), skiprows=4)   # y, u(x=0.5, y)
    vx2d = np.loadtxt(os.path.join(golden_dir, 'ldc_golden', 'vx2d'), skiprows=4)   # x, v(x, y=0.5)
    ok = np.isfinite(u_c)
    u_ref = np.interp(vy2d[:, 0], pos[ok], u_c[ok])
    sel = (vy2d[:, 0] > 0.02) & (vy2d[:, 0] < 0.98)
    err_u = np.max(np.abs(u_ref[sel] - vy2d[sel, 1]))
    ok = np.isfinite(v_c)
    v_ref = np.interp(vx2d[:, 0], pos[ok], v_c[ok])
    sel = (vx2d[:, 0] > 0.02) & (vx2d[:, 0] < 0.98)
    err_v = np.max(np.abs(v_ref[sel] - vx2d[sel, 1]))
    assert err_u < 0.03 and err_v < 0.03, (err_u, err_v)


def test_benchmark_mode_summary(capsys):
    """--mode=benchmark: TimeProfile accounting and the reference's summary lines (controller.py:740-765)."""
    cfg = dict(lat_nx=64, lat_ny=48, lat_nz=40, visc=0.05, subdomains=2, conn_axis='z', access_pattern='AA')
    ctrl = run_gpu('ldc_3d', 'LDCSim', 3, cfg, 260,
                   extra=dict(mode='benchmark', quiet=False, benchmark_sample_from=100, benchmark_minibatch=50))
    out = capsys.readouterr().out
    assert 'Subdomain 0: MLUPS eff:' in out and 'Subdomain 1: MLUPS eff:' in out and 'Total MLUPS: eff:' in out
    assert len(ctrl.timing_infos) == 2
    for ti, min_ti, max_ti, nodes in ctrl.timing_infos:
        assert ti.total > 0 and ti.comp > 0 and ti.bulk > 0 and ti.bnd > 0 and ti.coll > 0
        assert ti.comp <= ti.total * 1.5
        assert min_ti.total <= ti.total <= max_ti.total * (1 + 1e-9)
        assert ti.total_sq >= ti.total ** 2 * (1 - 1e-9)
    assert ctrl.runners[0]._profile.samples == 159      # iterations 100..258 (the final step is not sampled)
    assert ctrl.mlups_total > 0 and ctrl.mlups_comp >= ctrl.mlups_total * 0.5


def test_tools_merge_and_compare(tmp_path):
    """The reference's file-level checks run with its own tools: 2 subdomains merged == 1 subdomain, and
    AA == AB (tests/gpu/access_pattern.sh:12-29 + utils/compare_results.py), bit for bit."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from utils.compare_results import compare
    from utils.merge_subdomains import merge_subdomains
    from sailfish_amd import io
    cfg = dict(lat_nx=40, lat_ny=24, lat_nz=20, visc=0.03)
    one = str(tmp_path / 'one')
    two = str(tmp_path / 'two')
    ab = str(tmp_path / 'ab')
    run_gpu('ldc_3d', 'LDCSim', 3, dict(cfg, access_pattern='AA'), 60, extra=dict(output=one, every=30))
    run_gpu('ldc_3d', 'LDCSim', 3, dict(cfg, access_pattern='AA', subdomains=2, conn_axis='y'), 60,
            extra=dict(output=two, every=30))
    run_gpu('ldc_3d', 'LDCSim', 3, dict(cfg, access_pattern='AB'), 60, extra=dict(output=ab, every=30))
    digits = io.filename_iter_digits(60)
    for it in (30, 60):
        merge_subdomains(two, digits, it)
        merge_subdomains(one, digits, it)
        assert compare(io.merged_filename(one, digits, it), io.merged_filename(two, digits, it)) == 0
        assert compare(io.filename(one, digits, 0, it), io.filename(ab, digits, 0, it)) == 0


@pytest.mark.parametrize('module,sim,dim,cfg', [
    ('ldc_2d', 'LDCSim', 2, dict(lat_nx=48, lat_ny=40, visc=0.02)),
    ('poiseuille', 'PoiseuilleSim', 2, dict(lat_nx=32, lat_ny=24, visc=0.05, hip_fused_periodic=False)),
    ('ldc_3d', 'LDCSim', 3, dict(lat_nx=24, lat_ny=20, lat_nz=16, visc=0.03, model='mrt'))])
@pytest.mark.parametrize('pattern', ['AA', 'AB'])
def test_launch_graphs_equal_plain_stepping(module, sim, dim, cfg, pattern, tmp_path):
    """Stretches of steps without host interaction are replayed as HIP graphs of 16 / 2 steps
    (SubdomainRunner.fast_forward); output steps, odd remainders and the final step are normal steps.
    Same populations and the same output files as with --nohip_graphs."""
    res = {}
    for graphs in (True, False):
        out = str(tmp_path / ('g%d' % graphs))
        ctrl = run_gpu(module, sim, dim, dict(cfg, access_pattern=pattern), 75,
                       extra=dict(hip_graphs=graphs, output=out, every=37))
        r = ctrl.runners[0]
        assert r._sim.iteration == 75
        res[graphs] = (r._debug_get_dist(), np.load(out + '.0.37.npz')['rho'], np.load(out + '.0.74.npz')['rho'],
                       len(r.__dict__.get('_graphs', {})))
    assert res[True][3] >= 2 and res[False][3] == 0          # 16-step and 2-step graphs were built
    for a, b in zip(res[True][:3], res[False][:3]):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('bc', ['NTZouHeDensity', 'NTRegularizedDensity'])
def test_poiseuille_pressure_other_density_nodes(bc):
    """Pressure-driven channel with Zou-He / regularized density nodes instead of the equilibrium ones
    (reference examples/poiseuille.py `pressure_bc`; node types of boundary.mako:343-382, 487-506), through
    the whole host stack: set_node -> encoder -> type table -> kernels; against the oracle and the parabola."""
    from sailfish_amd import geo as geo_mod, node_type
    from sailfish_amd.controller import LBSimulationController
    cfg = dict(lat_nx=24, lat_ny=48, visc=0.1, horizontal=False, stationary=True, drive='pressure', wall='fullbb',
               force_implementation='guo', access_pattern='AA', max_iters=400, quiet=True, perf_stats_every=0)
    sim_cls = _host.load_sim_class('poiseuille', 'PoiseuilleSim')
    sim_cls.subdomain.pressure_bc = getattr(node_type, bc)
    ctrl = LBSimulationController(sim_cls, getattr(geo_mod, GEO[2]), default_config=dict(cfg))
    ctrl.run(ignore_cmdline=True)
    og = OracleGroup(sim_cls, 2, GEO[2], {k: v for k, v in cfg.items() if k not in ('max_iters', 'quiet', 'perf_stats_every')})
    og.run(400, save_last=True)
    r = ctrl.runners[0]
    rho_o = og.merged('rho')
    wet = np.isfinite(rho_o) & (rho_o != 0)
    assert np.max(np.abs(r._sim.rho[wet] - rho_o[wet]) / rho_o[wet]) < 1e-6
    assert np.max(np.abs(r._sim.v[1][wet] - og.merged('v1')[wet])) / 0.02 < 1e-6
    # physics: a channel flow of the right magnitude, symmetric across the channel (the density drop of the
    # example is calibrated for the equilibrium nodes and the flow is still developing after 400 steps)
    got = r._sim.v[1][24, :]
    assert 0.3 * sim_cls.subdomain.max_v < got.max() < 1.4 * sim_cls.subdomain.max_v
    assert np.max(np.abs(got[1:-1] - got[1:-1][::-1])) < 1e-4


@pytest.mark.parametrize('model,precision', [('bgk', 'double'), ('mrt', 'double'), ('bgk', 'single'), ('mrt', 'single')])
def test_poiseuille_error_curve_envelope(model, precision, golden_dir):
    """The reference's regression curve regtest/poiseuille.py: relative error of the maximum velocity of a
    127 x 128 force-driven channel (full-way bounce-back) after 100/visc iterations, 30 viscosities from
    1e-3 to 1e-1, against the numbers the reference recorded from its GPU path
    (tests/golden/poiseuille_curves/).  Recorded by an older revision => a two-sided bracket instead of equality: our
    error at the centre nodes may not be larger than the recorded one, and the recorded one may not be larger than
    ours one node off the centre (see below); single precision is compared where round-off does not dominate the
    recorded values (visc >= 0.02; they scatter by several 1e-3 there)."""
    data = np.loadtxt(os.path.join(golden_dir, 'poiseuille_curves', 'D2Q9_%s_force_%s_fullbb.dat' % (model, precision)))
    assert data.shape == (30, 2)
    sim_cls = _host.load_sim_class('poiseuille', 'PoiseuilleSim')
    rows = data if precision == 'double' else data[data[:, 0] >= 0.02]
    worst = 0.0
    for visc, recorded in rows[::3]:
        iters = 100 * (int(100 / visc) // 100)
        cfg = dict(lat_nx=127, lat_ny=128, visc=float(visc), horizontal=True, stationary=True, drive='force',
                   wall='fullbb', precision=precision, model=model, access_pattern='AA')
        ctrl = run_gpu('poiseuille', 'PoiseuilleSim', 2, cfg, iters)
        r = ctrl.runners[0]
        vx = r._sim.v[0]
        profile = vx[:, vx.shape[1] // 2]
        theory = sim_cls.subdomain.velocity_profile(r.config, np.arange(vx.shape[0]))
        err = np.nanmax(profile) / np.nanmax(theory) - 1.0
        # the other side of the bracket: the same measure ONE NODE OFF the centre-line pair (the channel is 126
        # lattice units wide between the half-way walls, the maximum sits between nodes 63 and 64).  The recorded
        # plateau, -2.516e-4 = -4 / 126^2 to 0.1 %, lies between the value at the centre nodes and the value one node
        # further out: that revision compared the same flow at a position up to one node away from where the current
        # regtest/poiseuille.py (and this test) samples it -- a difference of set-up, not of the scheme.
        centre = int(np.nanargmax(theory))
        off = min(profile[centre - 1], profile[centre + 2]) / np.nanmax(theory) - 1.0
        print('poiseuille %s %s visc %.5f: err %+.6e (one node off %+.6e) recorded %+.6e'
              % (model, precision, visc, err, off, recorded))
        if precision == 'double':
            assert abs(err) <= abs(recorded) + 5e-5, (visc, err, recorded)
            assert off - 5e-5 <= recorded <= err + 5e-5, (visc, off, recorded, err)
        else:       # the reference's single-precision record is round-off (it scatters by several 1e-3): one-sided
            assert abs(err) <= abs(recorded) + 1e-3, (visc, err, recorded)
        worst = max(worst, abs(err))
    assert worst < (3e-4 if precision == 'double' else 5e-3)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('nsub,axis,model', [(1, 'x', 'bgk'), (2, 'x', 'mrt'), (2, 'y', 'bgk')])
def test_indirect_addressing(pattern, nsub, axis, model):
    """--node_addressing=indirect (reference subdomain_runner.py:829-878): distributions stored for the
    active nodes only.  GPU == oracle twin (which tests/test_indirect_oracle.py shows to equal the dense
    run on every fluid node), and the distribution buffers shrink with the fill ratio."""
    cfg = dict(lat_nx=48, lat_ny=21, lat_nz=21, visc=0.05, periodic_x=True, grid='D3Q19', node_addressing='indirect',
               access_pattern=pattern, model=model, subdomains=nsub, conn_axis=axis)
    ctrl, exact = check_against_oracle('external_geometry', 'ExternalSimulation', 3, cfg, 25, 1e-4)
    assert exact
    for r in ctrl.runners:
        dense = int(np.prod(r._physical_size))
        assert r._dist_stride < 0.8 * dense and r._dist_stride >= r._subdomain.active_nodes + 1
        assert r._desc.node_addressing == 1
    v = merged_gpu(ctrl, 'v0')
    assert np.nanmax(v) > 1e-6


def test_gpu_invalid_value_check():
    """--check_invalid_results_gpu (reference geo_helpers.mako:193-213, default on): a sweep that meets a wet
    node with a non-finite density raises a flag on the device; the runner turns it into backend.FatalError with
    the position instead of writing garbage.  Switched off, the host-side check of the output catches it."""
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.backend_hip import HIPFatalError
    from sailfish_amd.controller import LBSimulationController
    base = _host.load_sim_class('ldc_2d', 'LDCSim')

    class Poisoned(base.subdomain):
        def initial_conditions(self, sim, hx, hy):
            base.subdomain.initial_conditions(self, sim, hx, hy)
            sim.vx[12, 10] = 1e20              # feq overflows -> inf - inf -> nan in the first sweep

    sim_cls = type('PoisonedSim', (base,), {'subdomain': Poisoned})
    cfg = dict(lat_nx=32, lat_ny=24, visc=0.05, access_pattern='AA', max_iters=20, quiet=True, perf_stats_every=0)
    with pytest.raises(HIPFatalError, match='Invalid value .*detected on the GPU: subdomain 0') as info:
        LBSimulationController(sim_cls, getattr(geo_mod, GEO[2]), default_config=dict(cfg)).run(ignore_cmdline=True)
    assert 'node (' in str(info.value)
    with pytest.raises(RuntimeError, match='Invalid value detected in output'):
        LBSimulationController(sim_cls, getattr(geo_mod, GEO[2]),
                               default_config=dict(cfg, check_invalid_results_gpu=False, output='/tmp/slf_poisoned')
                               ).run(ignore_cmdline=True)
    # a healthy run is not affected
    ctrl = run_gpu('ldc_2d', 'LDCSim', 2, dict(lat_nx=32, lat_ny=24, visc=0.05), 20)
    assert np.isfinite(ctrl.runners[0]._sim.rho[1:-1, 1:-1]).all()


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_poiseuille_force_edm(pattern):
    """--force_implementation=edm (exact difference method, reference relaxation_common.mako:66-99)."""
    cfg = dict(lat_nx=24, lat_ny=40, visc=0.05, horizontal=False, stationary=False, drive='force', wall='fullbb',
               force_implementation='edm', access_pattern=pattern)
    ctrl, exact = check_against_oracle('poiseuille', 'PoiseuilleSim', 2, cfg, 60, 0.02)
    assert exact
    assert ctrl.runners[0]._desc.force_implementation == 1


def test_sighup_triggers_checkpoint(tmp_path):
    """SIGHUP -> checkpoint at the next step (reference subdomain_runner.py:1528-1535)."""
    import signal
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    base = _host.load_sim_class('ldc_2d', 'LDCSim')

    class Hup(base):
        def after_step(self, runner):
            if self.iteration == 5:
                os.kill(os.getpid(), signal.SIGHUP)

    ck = str(tmp_path / 'hup')
    cfg = dict(lat_nx=32, lat_ny=24, visc=0.05, access_pattern='AA', max_iters=12, quiet=True, perf_stats_every=0,
               checkpoint_file=ck)
    old = signal.getsignal(signal.SIGHUP)
    try:
        LBSimulationController(Hup, getattr(geo_mod, GEO[2]), default_config=cfg).run(ignore_cmdline=True)
    finally:
        signal.signal(signal.SIGHUP, old)
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.cpoint.npz'))
    assert len(files) == 1 and '.06.' in files[0] or '.6.' in files[0], files
    assert 'dist0a' in np.load(os.path.join(str(tmp_path), files[0])).files


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('dim,cuts,size', [(2, [[9], [7]], (20, 16)), (3, [[5], [4], [3]], (11, 9, 7))])
def test_block_decomposition_on_gpu(pattern, dim, cuts, size):
    """2 x 2 (x 2) blocks of a periodic box, all on the one GPU: face, edge and corner halos and periodic images
    between different subdomains through LocalGroup; equal to the oracle group (tests/test_halo_oracle.py shows
    that one to equal the single-subdomain run)."""
    from sailfish_amd.controller import LBSimulationController
    from sailfish_amd.lb_single import LBFluidSim
    from sailfish_amd.subdomain import Subdomain2D, Subdomain3D
    from tests.test_halo_oracle import _block_geometry

    class Box(Subdomain2D if dim == 2 else Subdomain3D):
        def boundary_conditions(self, *h):
            pass

        def initial_conditions(self, sim, *h):
            sim.rho[:] = 1.0 + 0.01 * np.sin(2 * np.pi * h[0] / self.gx) * np.cos(2 * np.pi * h[1] / self.gy)
            sim.vx[:] = 0.03 * np.sin(2 * np.pi * h[1] / self.gy)
            sim.vy[:] = 0.02 * np.cos(2 * np.pi * h[0] / self.gx)

    class Sim(LBFluidSim):
        subdomain = Box

    cfg = dict(lat_nx=size[0], lat_ny=size[1], periodic_x=True, periodic_y=True, visc=0.02, model='mrt',
               access_pattern=pattern, grid='D2Q9' if dim == 2 else 'D3Q19')
    if dim == 3:
        cfg.update(lat_nz=size[2], periodic_z=True)
    geo_cls = _block_geometry(dim, cuts)
    og = OracleGroup(Sim, dim, geo_cls, dict(cfg))
    og.run(9, save_last=True)
    ctrl = LBSimulationController(Sim, geo_cls, default_config=dict(cfg, max_iters=9, quiet=True, perf_stats_every=0))
    ctrl.run(ignore_cmdline=True)
    assert len(ctrl.runners) == 2 ** dim
    fg, fo = merged_gpu(ctrl, 'dist'), og.merged('dist')
    assert np.array_equal(fg, fo, equal_nan=True)
    assert np.array_equal(merged_gpu(ctrl, 'rho'), og.merged('rho'))


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('steps', [7, 8])
@pytest.mark.parametrize('case', ['cavity_3x', 'pipe_2x', 'cavity_mrt_2x', 'cavity_64_rows'])
def test_x_slabs_through_face_buffers(pattern, steps, case):
    """1-D decompositions along x (the reference's default axis): the sweep's edge lanes write / read dense x-face
    buffers (sailfish_amd/xface.py, slf_module_set_xface_buffers) instead of ghost columns + pack / unpack kernels.
    Odd and even step counts (the two halo flavours of the in-place pattern), walls cut by the faces, and the same
    run with --nohip_xface: all equal to the oracle group bit for bit."""
    if case == 'cavity_3x':
        args = ('ldc_3d', 'LDCSim', 3, dict(lat_nx=30, lat_ny=12, lat_nz=10, visc=0.03, model='bgk', access_pattern=pattern,
                                            subdomains=3, conn_axis='x'))
        u = 0.05
    elif case == 'cavity_64_rows':      # 64 rows per plane: the rows of a launch are regrouped for the XCDs (xcd_row, slf_sweep.h)
        args = ('ldc_3d', 'LDCSim', 3, dict(lat_nx=24, lat_ny=64, lat_nz=6, visc=0.03, model='bgk', access_pattern=pattern,
                                            subdomains=2, conn_axis='x'))
        u = 0.05
    elif case == 'cavity_mrt_2x':
        args = ('ldc_3d', 'LDCSim', 3, dict(lat_nx=140, lat_ny=8, lat_nz=7, visc=0.03, model='mrt', access_pattern=pattern,
                                            subdomains=2, conn_axis='x'))
        u = 0.05
    else:
        args = ('poiseuille_3d', 'PoiseuilleSim', 3,
                dict(lat_nx=18, lat_ny=18, lat_nz=16, visc=0.1, flow_direction='z', stationary=False, drive='force',
                     force_implementation='guo', access_pattern=pattern, subdomains=2, conn_axis='x'))
        u = 0.02
    ctrl, exact = check_against_oracle(*args, steps, u)
    assert exact
    assert all(r._xface is not None for r in ctrl.runners)
    module, sim, dim, cfg = args
    plain = run_gpu(module, sim, dim, dict(cfg, hip_xface=False), steps)
    assert all(r._xface is None for r in plain.runners)
    assert np.array_equal(merged_gpu(ctrl, 'dist'), merged_gpu(plain, 'dist'), equal_nan=True)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_runner_with_placed_distribution_arrays(pattern, monkeypatch, tmp_path):
    """The runner's distribution arrays as placed buffers (physical chunks spread over HBM under one virtual range,
    sailfish_amd/placement.py; normally only for arrays >= 512 MiB): two subdomains, both access patterns, checkpoint
    round trip through host copies that cross chunk boundaries -- same numbers as the oracle."""
    from sailfish_amd import placement
    monkeypatch.setattr(placement, 'MIN_BYTES', 0)
    monkeypatch.setenv('SLF_PLACEMENT_SPAN_GIB', '1')
    cfg = dict(lat_nx=40, lat_ny=18, lat_nz=16, visc=0.03, model='bgk', access_pattern=pattern, subdomains=2, conn_axis='z')
    ctrl, exact = check_against_oracle('ldc_3d', 'LDCSim', 3, cfg, 21, 0.05)
    assert exact
    assert all(r.backend._placed for r in ctrl.runners)
    ck = str(tmp_path / 'ck')
    first = run_gpu('ldc_3d', 'LDCSim', 3, dict(cfg, subdomains=1), 11, extra=dict(checkpoint_file=ck, final_checkpoint=True))
    assert first.runners[0].backend._placed
    cp = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.cpoint.npz'))
    restored = run_gpu('ldc_3d', 'LDCSim', 3, dict(cfg, subdomains=1), 21,
                       extra=dict(restore_from=os.path.join(str(tmp_path), cp[0][:-len('.0.cpoint.npz')])))
    straight = run_gpu('ldc_3d', 'LDCSim', 3, dict(cfg, subdomains=1), 21)
    assert np.array_equal(restored.runners[0]._debug_get_dist(), straight.runners[0]._debug_get_dist(), equal_nan=True)
    for c in (ctrl, first, restored, straight):
        for r in c.runners:
            r.release()
            assert not r.backend._placed


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_minimize_roundoff_split_along_x(pattern):
    """--minimize_roundoff modules run the per-node kernels, which have no x-face buffers: a run split along
    x (the default axis) must take the ordinary halo links -- and equal the undivided run bit for bit."""
    cfg = dict(lat_nx=18, lat_ny=18, lat_nz=16, visc=0.1, flow_direction='z', stationary=False, drive='force',
               force_implementation='guo', access_pattern=pattern, minimize_roundoff=True, conn_axis='x')
    two = run_gpu('poiseuille_3d', 'PoiseuilleSim', 3, dict(cfg, subdomains=2), 8)
    assert all(r._xface is None for r in two.runners)
    one = run_gpu('poiseuille_3d', 'PoiseuilleSim', 3, dict(cfg, subdomains=1), 8)
    assert np.array_equal(merged_gpu(two, 'dist'), merged_gpu(one, 'dist'), equal_nan=True)
    assert np.array_equal(merged_gpu(two, 'rho'), merged_gpu(one, 'rho'), equal_nan=True)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_pressure_driven_channel_minimize_roundoff(pattern):
    """--minimize_roundoff with boundary-condition nodes (round 4): the pressure-driven channel of examples/poiseuille.py
    (NTEquilibriumDensity inlet / outlet, full-way bounce-back walls).  The run equals the oracle group bit for bit (same
    formulation on both sides), and its density delta / velocity equal the standard formulation's rho - 1 / u to f32
    round-off -- the formulation changes the arithmetic, not the model."""
    cfg = dict(lat_nx=24, lat_ny=40, visc=0.1, horizontal=False, stationary=True, drive='pressure', wall='fullbb',
               force_implementation='guo', access_pattern=pattern, minimize_roundoff=True)
    steps = 60
    ro = run_gpu('poiseuille', 'PoiseuilleSim', 2, cfg, steps)
    og = OracleGroup(_host.load_sim_class('poiseuille', 'PoiseuilleSim'), 2, GEO[2], cfg)
    og.run(steps, save_last=True)
    fg, fo = merged_gpu(ro, 'dist'), og.merged('dist')
    m = np.isfinite(fo)
    assert np.array_equal(fg[m], fo[m])
    std = run_gpu('poiseuille', 'PoiseuilleSim', 2, dict(cfg, minimize_roundoff=False), steps)
    rho_ro, rho = merged_gpu(ro, 'rho'), merged_gpu(std, 'rho')
    wet = ro.runners[0]._subdomain.fluid_map()          # nodes the sweep writes (the corner nodes of the inlet / outlet
    assert wet.sum() > 0.8 * wet.size                   # columns have no fluid neighbour: unused, they keep the initial field)
    assert np.max(np.abs((rho_ro[wet] + 1.0) - rho[wet])) < 2e-6
    for d in range(2):
        assert np.max(np.abs(merged_gpu(ro, 'v%d' % d)[wet] - merged_gpu(std, 'v%d' % d)[wet])) < 2e-6
    assert float(np.max(np.abs(merged_gpu(ro, 'v1')[wet]))) > 1e-4          # there is a flow


@pytest.mark.parametrize('stop_at', [5, 6])
def test_x_split_box_restored_at_odd_iteration(stop_at, tmp_path):
    """a fluid-only periodic box split along x (x-face buffers; the odd in-place step of its edge lanes does
    not pull out of the ghost columns), checkpointed at an ODD iteration, restored and continued: equal to the
    uninterrupted run bit for bit (the receive buffers are primed from the ghost columns of the restored state)."""
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    from sailfish_amd.lb_single import LBFluidSim
    from sailfish_amd.subdomain import Subdomain3D

    class PeriodicBox(Subdomain3D):
        def boundary_conditions(self, hx, hy, hz):
            pass

        def initial_conditions(self, sim, hx, hy, hz):
            sim.rho[:] = 1.0 + 1e-3 * np.sin(2 * np.pi * hx / self.gx)
            sim.vx[:] = 0.05 * np.sin(2 * np.pi * hy / self.gy)
            sim.vy[:] = 0.05 * np.sin(2 * np.pi * hz / self.gz)
            sim.vz[:] = 0.05 * np.sin(2 * np.pi * hx / self.gx)

    class BoxSim(LBFluidSim):
        subdomain = PeriodicBox

    cfg = dict(lat_nx=48, lat_ny=12, lat_nz=10, periodic_x=True, periodic_y=True, periodic_z=True, visc=0.02,
               access_pattern='AA', grid='D3Q19', subdomains=2, conn_axis='x', quiet=True, perf_stats_every=0)

    def run(steps, **extra):
        ctrl = LBSimulationController(BoxSim, geo_mod.EqualSubdomainsGeometry3D, default_config=dict(cfg, max_iters=steps, **extra))
        ctrl.run(ignore_cmdline=True)
        return ctrl

    total = 11
    straight = run(total)
    assert all(r._xface is not None and r._desc.fluid_only for r in straight.runners)
    ck = str(tmp_path / 'ck')
    run(stop_at, checkpoint_file=ck, final_checkpoint=True)
    restored = run(total, restore_from=ck + '.last')
    assert all(r._sim.iteration == total for r in restored.runners)
    assert np.array_equal(merged_gpu(restored, 'dist'), merged_gpu(straight, 'dist'))
    assert np.array_equal(merged_gpu(restored, 'rho'), merged_gpu(straight, 'rho'))


def _masked_equal(a, b):
    m = np.isfinite(a)
    return np.array_equal(m, np.isfinite(b)) and np.array_equal(a[m], b[m])


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('addressing', ['direct', 'indirect'])
@pytest.mark.parametrize('nsub,vertical', [(2, False), (3, False), (2, True), (3, True)])
def test_cylinder_subdomains(pattern, addressing, nsub, vertical):
    """The reference's regtest/subdomains/2d_cylinder.py (flow past a cylinder, examples/cylinder.py, cut into 2 or 3
    subdomains along the flow, lying and standing, both access patterns, both addressing modes): the run equals the
    single-subdomain run -- here bit for bit, fields and populations -- and the oracle twin of the same decomposition."""
    size = dict(lat_nx=36, lat_ny=60) if vertical else dict(lat_nx=60, lat_ny=36)
    cfg = dict(size, visc=0.1, vertical=vertical, access_pattern=pattern, node_addressing=addressing,
               force_implementation='guo')
    split = dict(cfg, subdomains=nsub, conn_axis='y' if vertical else 'x')
    ctrl, exact = check_against_oracle('cylinder', 'CylinderSimulation', 2, split, 40, 1e-4)
    assert exact
    one = run_gpu('cylinder', 'CylinderSimulation', 2, dict(cfg, subdomains=1), 40)
    for what in ('rho', 'v0', 'v1', 'dist'):
        assert _masked_equal(merged_gpu(ctrl, what), merged_gpu(one, what)), what
    assert np.nanmax(np.abs(merged_gpu(one, 'v1' if vertical else 'v0'))) > 1e-5       # the force drives a flow


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('addressing', ['direct', 'indirect'])
@pytest.mark.parametrize('nsub,axis', [(2, 'x'), (2, 'z')])
def test_sphere_subdomains(pattern, addressing, nsub, axis):
    """regtest/subdomains/3d_sphere.py: flow past a sphere in a duct (examples/sphere_3d.py), two subdomains against one
    (the reference cuts along x; here across the flow as well)."""
    cfg = dict(lat_nx=40, lat_ny=21, lat_nz=24, visc=0.01, access_pattern=pattern, node_addressing=addressing,
               force_implementation='guo')
    split = dict(cfg, subdomains=nsub, conn_axis=axis)
    ctrl, exact = check_against_oracle('sphere_3d', 'SphereSimulation', 3, split, 30, 1e-4)
    assert exact
    one = run_gpu('sphere_3d', 'SphereSimulation', 3, dict(cfg, subdomains=1), 30)
    for what in ('rho', 'v0', 'v1', 'v2', 'dist'):
        assert _masked_equal(merged_gpu(ctrl, what), merged_gpu(one, what)), what
    assert np.nanmax(np.abs(merged_gpu(one, 'v0'))) > 1e-5


@pytest.mark.parametrize('pattern', ['AA', 'AB'])
@pytest.mark.parametrize('case', ['2d', '2d_y2', '2d_x2', '3d', '3d_z2', '3d_y2'])
def test_do_nothing_outlet_through_the_runner(pattern, case):
    """The set-up of the reference's tests/gpu/do_nothing_node.py (and a duct with the outlet on a z face) through the
    whole host stack -- set_node(NTDoNothing) -> encoder -> type table (a do-nothing kind in place, a fluid node in the
    two-copy pattern) -> kernels -- against the oracle twin, one subdomain and two (the outlet column then crosses the seam,
    or lies in the second subdomain)."""
    from tests import _open_sims as S
    nsub, axis = (2, case[-2]) if '_' in case else (1, 'x')
    if case.startswith('2d'):
        cfg = dict(lat_nx=64, lat_ny=40, visc=0.05, access_pattern=pattern, subdomains=nsub, conn_axis=axis)
        _, exact = check_against_oracle(S.OpenChannelSim, None, 2, cfg, 61, 0.05)
    else:
        cfg = dict(lat_nx=20, lat_ny=14, lat_nz=24, visc=0.05, periodic_x=True, access_pattern=pattern, subdomains=nsub,
                   conn_axis=axis)
        _, exact = check_against_oracle(S.OpenDuctSim, None, 3, cfg, 40, 0.04)
    assert exact


def test_do_nothing_outlet_in_place_equals_the_two_copy_run_on_the_gpu():
    """The reference's own assertion (tests/gpu/do_nothing_node.py: 64 x 64, 1000 steps, AB against AA with
    numpy.testing.assert_allclose) -- here the fields are the same to the bit."""
    from tests import _open_sims as S
    cfg = dict(lat_nx=64, lat_ny=64, visc=0.05)
    fields = {}
    for pattern in ('AB', 'AA'):
        ctrl = run_gpu(S.OpenChannelSim, None, 2, dict(cfg, access_pattern=pattern), 1000)
        sim = ctrl.runners[0]._sim
        fields[pattern] = [sim.rho.copy(), sim.vx.copy(), sim.vy.copy()]
    for a, b in zip(fields['AB'], fields['AA']):
        np.testing.assert_allclose(a, b)
        assert np.array_equal(a, b, equal_nan=True)
    # the outlet lets the flow through: the last fluid column still moves at about the inlet speed
    assert 0.03 < np.nanmean(fields['AA'][1][1:-1, -1]) < 0.07


@pytest.mark.parametrize('pattern', ['AA', 'AB'])
@pytest.mark.parametrize('case', ['2d', '2d_y2', '3d', '3d_x2'])
def test_slip_walls_through_the_runner(pattern, case):
    """NTSlip(orientation=...) through the host stack against the oracle twin: a force-driven flow between two slip walls."""
    from tests import _open_sims as S
    nsub, axis = (2, case[-2]) if '_' in case else (1, 'x')
    if case.startswith('2d'):
        cfg = dict(lat_nx=70, lat_ny=24, visc=0.05, periodic_x=True, force_implementation='guo', access_pattern=pattern,
                   subdomains=nsub, conn_axis=axis)
        _, exact = check_against_oracle(S.SlipChannelSim, None, 2, cfg, 80, 1e-3)
    else:
        cfg = dict(lat_nx=20, lat_ny=12, lat_nz=10, visc=0.05, periodic_x=True, periodic_z=True, force_implementation='guo',
                   access_pattern=pattern, subdomains=nsub, conn_axis=axis)
        _, exact = check_against_oracle(S.SlipDuctSim, None, 3, cfg, 60, 1e-3)
    assert exact


def _pulsating_channel(dim):
    """An open channel whose inlet / outlet densities oscillate in time and whose inlet ... (node_type.DynamicValue)."""
    import sympy
    from sailfish_amd import node_type as nt
    from sailfish_amd import sym
    from sailfish_amd.lb_single import LBFluidSim
    from sailfish_amd.subdomain import Subdomain2D, Subdomain3D
    S = sym.S
    amp, om = 0.004, 2 * np.pi / 60.0

    class Channel(Subdomain2D if dim == 2 else Subdomain3D):
        def boundary_conditions(self, hx, hy, *hz):
            wall = (hy == 0) | (hy == self.gy - 1)
            self.set_node(wall, nt.NTFullBBWall)
            # a density that depends on time at the inlet, on time AND position at the outlet (an entry per node)
            self.set_node((hx == 0) & ~wall, nt.NTEquilibriumDensity(nt.DynamicValue(1.0 + amp * sympy.sin(S.time * om))))
            self.set_node((hx == self.gx - 1) & ~wall,
                          nt.NTEquilibriumDensity(nt.DynamicValue(1.0 - amp * sympy.sin(S.time * om) * (1 + 0.01 * S.gy))))

        def initial_conditions(self, sim, hx, hy, *hz):
            sim.rho[:] = 1.0

    class ChannelSim(LBFluidSim):
        subdomain = Channel

        @classmethod
        def modify_config(cls, config):
            if dim == 3:
                config.periodic_z = True
    return ChannelSim


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('dim,nsub,axis', [(2, 1, 'x'), (2, 2, 'y'), (3, 1, 'x'), (3, 2, 'x')])
def test_time_dependent_boundary_values(pattern, dim, nsub, axis):
    """Boundary values that depend on time (and position): evaluated on the host before every step and written into the
    kernels' parameter table on the calc stream (slf_module_update_node_params) -- the HIP run equals the oracle twin,
    which takes the same values, bit for bit; one and two subdomains, both access patterns, step plans in use."""
    size = dict(lat_nx=24, lat_ny=11) if dim == 2 else dict(lat_nx=70, lat_ny=9, lat_nz=6)
    cfg = dict(size, visc=0.08, access_pattern=pattern, subdomains=nsub, conn_axis=axis)
    ctrl, exact = check_against_oracle(_pulsating_channel(dim), None, dim, cfg, 37, 0.01)
    assert exact
    assert all(r._time_dependent() for r in ctrl.runners)


def _pulsating_face(dim=3):
    """A duct along z, periodic along x and y, whose inlet covers the whole face z = 0 with a density that depends on time
    AND on both in-plane coordinates: one entry of the parameter table per node of the face, all in one update range."""
    import sympy
    from sailfish_amd import node_type as nt
    from sailfish_amd import sym
    from sailfish_amd.lb_single import LBFluidSim
    from sailfish_amd.subdomain import Subdomain3D
    S = sym.S
    amp, om = 0.004, 2 * np.pi / 7.0

    class Duct(Subdomain3D):
        def boundary_conditions(self, hx, hy, hz):
            self.set_node(hz == 0, nt.NTEquilibriumDensity(nt.DynamicValue(
                1.0 + amp * sympy.sin(S.time * om) * (1 + 0.01 * S.gx) * (1 - 0.02 * S.gy))))
            self.set_node(hz == self.gz - 1, nt.NTEquilibriumDensity(1.0))

        def initial_conditions(self, sim, hx, hy, hz):
            sim.rho[:] = 1.0

    class DuctSim(LBFluidSim):
        subdomain = Duct
    return DuctSim


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('nx,ny', [(13, 15), (14, 14), (13, 18)])
def test_long_parameter_updates(nx, ny, pattern, precision):
    """slf_module_update_node_params on both sides of its 256 entries (slf_api.hip: PARAM_UPDATE_MAX): up to there the
    values travel as kernel arguments, beyond it through a ring of four pinned staging buffers.  Faces of 255, 256 and
    300 nodes (the ghost nodes around the periodic face have entries too), eleven steps -- every staging buffer is used at
    least twice, with other values --, bit-identical to the oracle twin, which takes the same values."""
    n = (nx + 2) * (ny + 2)
    assert n in (255, 256, 300)
    cfg = dict(lat_nx=nx, lat_ny=ny, lat_nz=8, visc=0.08, access_pattern=pattern, precision=precision, periodic_x=True,
               periodic_y=True)
    ctrl, exact = check_against_oracle(_pulsating_face(), None, 3, cfg, 11, 0.01)
    assert exact
    r, = ctrl.runners
    assert r._time_dependent()
    enc = r._subdomain._encoder
    updates = enc.dynamic_updates(0)
    assert [len(values) for first, values in updates] == [n]
    # the values differ from node to node and from step to step
    assert len(np.unique(enc.dynamic_updates(3)[0][1])) > n // 2
    assert all(not np.array_equal(enc.dynamic_updates(it)[0][1], enc.dynamic_updates(it + 4)[0][1]) for it in range(1, 7))
    assert np.nanmax(np.abs(merged_gpu(ctrl, 'v2'))) > 1e-5
    r.release()


def test_womersley_flow_follows_the_analytical_profile():
    """examples/womersley.py: a pipe driven by dP(t) = dP0 sin(omega t) through time-dependent equilibrium-density
    nodes.  After seven periods (the start-up transient decays with the slowest viscous mode, nu 2.405^2 / R^2 = 1 / 4400
    steps) the axial velocity across the middle of the pipe, sampled at four phases of the eighth period, follows the classical Womersley solution (amplitude and phase lag; staircase walls, weak compressibility and
    the finite pipe leave under one per cent of the peak amplitude)."""
    sim_cls = _host.load_sim_class('womersley', 'WomersleySim')
    omega, nx, d = 0.002, 96, 34
    period = 2 * np.pi / omega
    errs = []
    for phase in (0.0, 0.25, 0.5, 0.75):
        steps = int(round((7 + phase) * period))
        ctrl = run_gpu(sim_cls, None, 3, dict(lat_nx=nx, lat_ny=d, lat_nz=d, visc=0.01, omega=omega, access_pattern='AA',
                                              drive='pressure', subdomains=1), steps)
        r = ctrl.runners[0]
        vx = np.asarray(r._sim.vx)[d // 2, :, nx // 2]                 # across the pipe, through its axis
        sd = r._subdomain
        width = sd.channel_width(r.config)
        y = np.arange(d, dtype=np.float64)
        rad = np.abs(y - (d / 2 - 0.5)) / (width / 2.0)
        inside = rad < 0.95
        want = sd.womersley_profile(rad[inside], steps)
        got = vx[inside]
        scale = np.max(np.abs(sd.womersley_profile(np.linspace(0, 0.95, 20)[:, None], np.linspace(0, period, 40)[None, :])))
        errs.append(float(np.max(np.abs(got - want)) / scale))
        for rr in ctrl.runners:
            rr.release()
    print('Womersley profile, max deviation / peak amplitude at four phases:', ['%.3f' % e for e in errs])
    assert max(errs) < 0.03, errs          # measured: 0.005 - 0.009


@pytest.mark.parametrize('drive,pattern,nsub', [('force', 'AA', 1), ('force', 'AB', 2), ('pressure', 'AA', 2), ('pressure', 'AB', 1)])
def test_pulsatile_example_equals_the_oracle(drive, pattern, nsub):
    """examples/poiseuille_pulsatile.py (cf. the reference's example of the same name): a body force resp. a pressure
    difference a0 sin(t), t = iteration x dt_per_lattice_time_unit -- the force as an argument of the sweep launches
    (slf_module_set_body_force before every step), the densities through the parameter table."""
    cfg = dict(lat_nx=40, lat_ny=18, visc=0.05, drive=drive, horizontal=True, access_pattern=pattern, dt_per_lattice_time_unit=0.05,
               wall='fullbb', stationary=False, subdomains=nsub, conn_axis='x')
    ctrl, exact = check_against_oracle('poiseuille_pulsatile', 'PulsatileSim', 2, cfg, 41, 0.02)
    assert exact and all(r._time_dependent() for r in ctrl.runners)
