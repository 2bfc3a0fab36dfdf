"""Force objects on the host (no GPU): link detection pinned to the reference, the runner's index tables against the
meaning of the arrays (tests/_force_twin.py) on CPU-oracle runs, momentum balance, and the public surface through
LBSimulationController with the CPU test backend (tests/_force_backend.py)."""
import math
import os

import numpy as np
import pytest

from sailfish_amd import hipabi
from tests import _force_sims as fs
from tests import _force_twin as tw
from tests import _host
from tests._force_backend import ForceOracleBackend
from tests._oracle_group import OracleGroup

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'force_objects.npz')
CASES = {'cylinder': (fs.cylinder_sim, 2, fs.CYLINDER, fs.CYLINDER_BOX), 'sphere': (fs.sphere_sim, 3, fs.SPHERE, fs.SPHERE_BOX)}
GEO = {2: 'EqualSubdomainsGeometry2D', 3: 'EqualSubdomainsGeometry3D'}
STEPS = 50


# ---- 1. get_fo_distributions pinned to the reference -----------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_get_fo_distributions_equals_the_reference(name):
    """tests/golden/force_objects.npz (tools/capture_force_objects.py): the reference's Subdomain.get_fo_distributions() for
    an interior box around the cylinder / the sphere.  Same node map, same direction set, same coordinates in the same
    order."""
    simf, dim, base, box = CASES[name]
    g = np.load(GOLDEN)
    assert dict(zip(g[name + '_cfg_keys'].tolist(), g[name + '_cfg_vals'].tolist())) == \
        dict((k, v) for k, v in base.items() if k.startswith('lat_n'))
    assert tuple(g[name + '_start']) == tuple(box[0]) and tuple(g[name + '_end']) == tuple(box[1])
    _, _, (r,) = _host.build_runners(simf(), dim, None, dict(base))
    r._init_geometry()
    sub = r._subdomain
    assert np.array_equal(sub.visualization_map(), g[name + '_vis_map'])
    got = sub.get_fo_distributions(r._sim.force_objects[0])
    assert sorted(got) == g[name + '_dirs'].tolist()
    for i, locs in got.items():
        assert len(locs) == dim
        assert np.array_equal(np.stack(locs), g['%s_d%d' % (name, i)]), i
    assert sub.fo_links_leaving(r._sim.force_objects[0]) is None


# ---- 2. - 4. the runner's tables against the meaning of the arrays; AA == AB; dense == indirect ---------------------------
def _tables(sub):
    """The runner's link tables for the oracle subdomain `sub` (no device: the CPU test backend keeps them on the host)."""
    r = sub.runner
    r._desc, r._dist_stride, r.backend, r.module = sub.desc, hipabi.dist_stride(sub.desc), ForceOracleBackend(), None
    if sub.indirect:
        r._host_indirect_address = sub.addr
    r._init_force_objects()
    return r._fo_tables


def _histories(name):
    simf, dim, base, box = CASES[name]
    out = {}
    for pattern in ('AB', 'AA'):
        for addressing in ('direct', 'indirect'):
            og = OracleGroup(simf(), dim, GEO[dim], dict(base, access_pattern=pattern, node_addressing=addressing,
                                                         precision='double'))
            (s,) = og.subs
            grid, vis = s.runner._sim.grid, s.runner._subdomain.visualization_map()
            t = _tables(s)
            idx, idx2, dirs, seg = t['host']
            assert t['n'] == 1 and seg.tolist() == [0, len(idx)]
            meaning, table = [], []
            for k in range(STEPS):
                og.step()
                odd = pattern == 'AA' and (s.iteration & 1) == 1
                meaning.append(tw.force_on_box(og.merged('dist'), vis, (0,) * dim, box[0], box[1], grid, odd))
                cur = s.dist[0] if s.aa else s.dist[s.iteration & 1]
                table.append(tw.fsum_force(tw.link_terms(s.raw(cur), idx, idx2, dirs, grid)))
            out[pattern, addressing] = (np.array(meaning), np.array(table), (idx, idx2, dirs))
    return out


_cache = {}


@pytest.fixture(params=sorted(CASES))
def histories(request):
    if request.param not in _cache:
        _cache[request.param] = _histories(request.param)
    return request.param, _cache[request.param]


def test_runner_tables_read_the_post_propagation_populations(histories):
    """Every step of 50, both patterns (the in-place one at both parities), both addressing modes: the sum over the
    runner's (idx, idx2, dirs) tables == the twin that finds the links on the node map and reads dist[opp(i)][s] +
    dist[i][f] where the access pattern keeps those post-propagation values.  Exactly (math.fsum of the same terms)."""
    name, h = histories
    for key, (meaning, table, _) in h.items():
        assert np.isfinite(meaning).all() and np.array_equal(meaning, table), (name, key)
        assert meaning[-1][0] > 0 and abs(meaning[-1][1]) < 1e-3 * meaning[-1][0], (name, key)     # along the flow


def test_link_order_does_not_depend_on_pattern_or_addressing(histories):
    name, h = histories
    ref = h['AB', 'direct'][2][2]
    for key, (_, _, (idx, idx2, dirs)) in h.items():
        assert np.array_equal(dirs, ref) and np.all(np.diff(dirs.astype(int)) >= 0), (name, key)
    # dense tables: the same words in both patterns
    for a in (0, 1):
        assert np.array_equal(h['AB', 'direct'][2][a], h['AA', 'direct'][2][a])


def test_in_place_equals_two_copy_bit_for_bit_at_every_step(histories):
    name, h = histories
    for addressing in ('direct', 'indirect'):
        assert np.array_equal(h['AA', addressing][1], h['AB', addressing][1]), (name, addressing)


def test_indirect_equals_dense_bit_for_bit_at_every_step(histories):
    name, h = histories
    for pattern in ('AB', 'AA'):
        assert np.array_equal(h[pattern, 'indirect'][1], h[pattern, 'direct'][1]), (name, pattern)


# ---- 5. momentum balance -------------------------------------------------------------------------------------------------
def test_momentum_balance_of_the_forced_channel():
    """Cylinder channel 48 x 30, double, 3000 steps: at steady state the walls and the cylinder together take up the
    momentum the body force puts in, F_x(all solids) = a sum(rho over the fluid nodes), and F_y = 0.  (The box is the whole
    domain: its links wrap around the periodic x axis, which the twin follows; the product refuses such links.)

    Measured with the CPU oracle: F_x = 1.27499974e-02 against 1.27500002e-02, relative difference 2.23e-7 (8.0e-14 after
    6000 steps: the flow is still settling), |F_y| / F_x = 1.54e-10.  Tolerances = 10 x measured: 2.3e-6 and 1.6e-9."""
    og = OracleGroup(fs.cylinder_sim(), 2, GEO[2], dict(fs.CYLINDER, access_pattern='AB', precision='double'))
    og.run(3000, save_last=False)
    (s,) = og.subs
    vis = s.runner._subdomain.visualization_map()
    real = og.merged('dist')
    f = tw.force_on_box(real, vis, (0, 0), (0, 0), (47, 29), s.runner._sim.grid, False)
    drive = s.runner._sim.acceleration * math.fsum(real.sum(axis=0)[vis == 0])
    print('F = %r, a sum rho = %.9e, relative difference %.3e, |Fy| / Fx %.3e' % (f, drive, (f[0] - drive) / drive,
                                                                              abs(f[1]) / f[0]))
    assert abs(f[0] - drive) <= 2.3e-6 * drive
    assert abs(f[1]) <= 1.6e-9 * f[0]


# ---- 6. through LBSimulationController with the CPU test backend ---------------------------------------------------------
WALL_BOX = ((30, 0), (40, 0))       # a stretch of the lower wall: links up into the channel only
FLUID_BOX = ((3, 10), (6, 12))      # no solid node
EDGE_BOX = ((0, 0), (5, 0))         # lower wall next to the periodic x face: (0, 0) -> (-1, 1) is fluid across it


def _control(sim_cls, dim, cfg, steps=7):
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    ctrl = LBSimulationController(sim_cls, getattr(geo_mod, GEO[dim]),
                                  default_config=dict(cfg, max_iters=steps, quiet=True, perf_stats_every=0, gpus=[0],
                                                      backends='tests._force_backend', output=''))
    ctrl.run(ignore_cmdline=True)
    return ctrl


def _hook(log):
    """after_step of the reference's examples/square_cylinder_2d.py, recording (subdomain, iteration, object id, force(),
    twin on the runner's populations)."""
    def hook(sim, runner):
        runner.update_force_objects()
        sub, sp = runner._subdomain, runner._spec
        real = runner._debug_get_dist()[(slice(None),) + tuple(sp._nonghost_slice)]
        odd = sim.config.access_pattern == 'AA' and (sim.iteration & 1) == 1
        for fo in sim.force_objects:
            if not fo.initialized:
                log.append((sp.id, sim.iteration, fo.id, None, None))
                continue
            runner.backend.from_buf(fo.gpu_force_buf)
            got = fo.force()
            assert len(got) == sim.dim and all(type(x) is float for x in got) and fo.force_buf.shape == (sim.dim,)
            twin = tw.force_on_box(real, sub.visualization_map(), sp.location, fo.start, fo.end, sim.grid, odd)
            log.append((sp.id, sim.iteration, fo.id, got, twin[:sim.dim]))
    return hook


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_two_objects_and_one_without_links_through_the_controller(pattern, addressing='direct'):
    """(Dense arrays: the CPU test backend has no indirect addressing.  Indirect tables: the oracle runs above, and
    tests/test_gpu_force_objects.py through the controller on the device.)"""
    log = []
    sim_cls = fs.cylinder_sim((fs.CYLINDER_BOX, FLUID_BOX, WALL_BOX), _hook(log))
    ctrl = _control(sim_cls, 2, dict(fs.CYLINDER, access_pattern=pattern, node_addressing=addressing, precision='double'))
    sim = ctrl.runners[0]._sim
    assert [fo.id for fo in sim.force_objects] == [0, 1, 2]
    assert [fo.initialized for fo in sim.force_objects] == [True, False, True]
    assert sim.force_objects[1].gpu_force_buf is None and sim.force_objects[1].force_buf is None
    assert len(log) == 7 * 3 and sorted(set(e[1] for e in log)) == list(range(1, 8))
    for sid, it, oid, got, twin in log:
        assert (got is None) == (oid == 1)
        if got is not None:
            assert got == twin and got[0] != 0.0, (it, oid)
    # the wall stretch is pushed along the flow and down (the pressure of the fluid above it)
    last = [e for e in log if e[1] == 7 and e[2] == 2][0][3]
    assert last[0] > 0 and last[1] < 0


def test_single_precision_sphere_through_the_controller():
    log = []
    ctrl = _control(fs.sphere_sim(hook=_hook(log)), 3, dict(fs.SPHERE, access_pattern='AA', precision='single'), steps=5)
    assert ctrl.runners[0]._sim.force_objects[0].num_links == 514
    assert len(log) == 5 and all(got == twin for _, _, _, got, twin in log)


def test_object_inside_one_of_two_subdomains_is_initialised_there_only():
    log = []
    ctrl = _control(fs.cylinder_sim((WALL_BOX,), _hook(log)), 2,
                    dict(fs.CYLINDER, access_pattern='AB', precision='double', subdomains=2, conn_axis='x'))
    assert len(ctrl.runners) == 2
    r0, r1 = sorted(ctrl.runners, key=lambda r: r._spec.id)
    assert r0._sim is not r1._sim               # a simulation object, and so force objects, per runner
    assert not r0._sim.force_objects[0].initialized and r0._fo_tables is None
    assert r1._sim.force_objects[0].initialized and r1._spec.location[0] == 24
    for sid, it, oid, got, twin in log:
        assert (got is None) == (sid == r0._spec.id)
        if got is not None:
            assert got == twin
    # ... and the same numbers as the undivided run
    one = []
    _control(fs.cylinder_sim((WALL_BOX,), _hook(one)), 2, dict(fs.CYLINDER, access_pattern='AB', precision='double'))
    assert [e[3] for e in log if e[3] is not None] == [e[3] for e in one]


@pytest.mark.parametrize('boxes,cfg,face', [
    ((fs.CYLINDER_BOX,), dict(subdomains=2, conn_axis='x'), 'x_high'),      # the seam at x = 24 cuts the cylinder
    ((EDGE_BOX,), dict(), 'x_low'),                                          # fluid on both sides of the periodic face
])
def test_links_that_leave_the_subdomain_are_refused(boxes, cfg, face):
    with pytest.raises(NotImplementedError, match=r'ForceObject\(id=0\).*face %s' % face):
        _control(fs.cylinder_sim(boxes), 2, dict(fs.CYLINDER, access_pattern='AB', precision='double', **cfg))


def test_box_that_touches_a_wall_edge_of_the_domain_is_fine():
    """The whole lower wall of a channel that is NOT periodic: its end nodes touch the domain edge, beyond which there is
    nothing (and the wrapped neighbour is a wall node)."""
    from tests import _indirect_sims
    from sailfish.lb_base import ForceObject
    base = _indirect_sims.make_sim(2, inlet='NTRegularizedVelocity', outlet='NTZouHeDensity')

    class Sim(base):
        def __init__(self, config):
            super(Sim, self).__init__(config)
            self.add_force_object(ForceObject((0, 0), (39, 0)))      # (the alias with the spelling put right)

    ctrl = _control(Sim, 2, dict(lat_nx=40, lat_ny=14, visc=0.05, precision='double'))
    fo = ctrl.runners[0]._sim.force_objects[0]
    assert fo.initialized and fo.num_links > 0


def test_shan_chen_simulations_are_refused():
    from sailfish.lb_base import ForceObject
    from examples.sc_phase_separation import PhaseSeparationSim

    class Sim(PhaseSeparationSim):
        def __init__(self, config):
            super(Sim, self).__init__(config)
            self.add_force_oject(ForceObject((2, 2), (5, 5)))

    with pytest.raises(NotImplementedError, match='single-fluid'):
        _control(Sim, 2, dict(lat_nx=16, lat_ny=16, precision='double'))
