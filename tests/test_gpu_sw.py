"""The shallow-water model (LBFreeSurface; the SW instantiations of the per-node sweep and of SetInitialConditions,
csrc/slf_kernels.hip, csrc/slf_plain.h) on the GPU: against its numpy twin (tests/_sw_twin.py, itself held against the
reference's expression objects by tests/test_sw_twin.py), against itself across configurations, and against the physics
-- the water volume stays put and a gravity wave travels at sqrt(g h0).  Tolerances are sized from the twin -- the twin in
the kernels' format against the twin in the next wider one, times ORDER_FACTOR as in tests/test_gpu_fe.py -- never from what
the kernels return."""
import os
import runpy
import sys

import numpy as np
import pytest

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish_amd import hipabi
from sailfish_amd.box import BoxSim
from sailfish_amd.node_type import DynamicValue
from sailfish_amd.sym import S
from tests import _sw
from tests import _sw_twin as tw
from tests._lat import merged

pytestmark = pytest.mark.gpu

ORDER_FACTOR = 4      # what another summation order may cost over the twin's own rounding error
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _diff(a, b):
    """The largest difference between two arrays where both are finite (never-written slots are NaN in both)."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    return float(np.max(np.abs(a[ok] - b[ok]))) if ok.any() else 0.0


def twin_step_with_error(box):
    """One step of the twin box (fields stored) and what it is worth: the same step from the same state in the next wider
    format, the largest difference in the populations and in rho / v.  Periodic axes wrapped in-sweep only (the ghost-layer
    kernels move data; their runs are compared bit for bit with these)."""
    assert not box.pbc_axes
    R = box.dtype
    wide = tw.wider(R)
    it = box.iteration
    if wide is None:      # no wider format: a step is some 80 roundings per population, each half an ulp of values below 2
        box.step(save_macro=True)
        e = 80 * float(np.finfo(R).eps)
        return e, e
    wt = tw.SwTwin(box.desc, R=wide)
    if box.accel_field is not None:
        wt.set_accel_field(box.accel_field.astype(wide))
    if box.aa:
        prop, src, dst = (2 if (it & 1) else 1), 0, 0
    else:
        prop, src, dst = 0, it & 1, 1 - (it & 1)
    din = box.dist[src].astype(wide)
    dout = din if box.aa else box.dist[dst].astype(wide)
    fields = [a.astype(wide) for a in (box.rho, box.v[0], box.v[1])]      # (dry nodes keep what they hold)
    wt.step(prop, box.node_map, din, dout, fields[0], fields[1], fields[2], None, 1)
    box.step(save_macro=True)
    ef = _diff(box.dist[dst], dout)
    em = max(_diff(a, b) for a, b in zip([box.rho, box.v[0], box.v[1]], fields))
    return ef, em


def run_against_twin(backend, desc, periodic, nmap, fields, steps, accel_field=None, per_step=None):
    """`steps` steps on the GPU and on the twin; after every one the populations and rho / v within ORDER_FACTOR times the
    twin's own error, summed over the steps so far.  per_step(step, gpu, twin): called before each step."""
    twin = _sw.start(tw.SwTwinBox(desc, periodic, nmap, accel_field=accel_field), fields)
    gpu = BoxSim(backend, desc, periodic=periodic, node_map=nmap, accel_field=accel_field, accel_field_fill=np.nan)
    worst = 0.0
    try:
        _sw.start(gpu, fields)
        assert _diff(gpu.real_view(gpu.get_dist()), twin.real_view(twin.current_dist())) <= \
            ORDER_FACTOR * 16 * np.finfo(gpu.dtype).eps      # SetInitialConditions
        tol_f = tol_m = 0.0
        for step in range(steps):
            if per_step is not None:
                per_step(step, gpu, twin)
            ef, em = twin_step_with_error(twin)
            tol_f += ORDER_FACTOR * ef
            tol_m += ORDER_FACTOR * em
            gpu.step(save_macro=True)
            df = _diff(gpu.real_view(gpu.get_dist()), twin.real_view(twin.current_dist()))
            rho, v = gpu.fetch_fields()
            dm = max(_diff(gpu.real_view(a), twin.real_view(b)) for a, b in zip([rho, v[0], v[1]], [twin.rho, twin.v[0], twin.v[1]]))
            print('step %d: populations differ by %.3e (bound %.3e), fields by %.3e (bound %.3e)' % (step, df, tol_f, dm, tol_m))
            assert df <= tol_f and dm <= tol_m, (step, df, tol_f, dm, tol_m)
            worst = max(worst, df)
        assert np.all(np.isfinite(gpu.real_view(gpu.get_dist())))
    finally:
        gpu.release()
    return twin, worst


# ---- one collision ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [0, 1], ids=['g=0.001', 'g=0.05'])
@pytest.mark.parametrize('precision', ['single', 'double'])
def test_one_collision_against_the_twin(backend, golden_dir, precision, k):
    """A periodic 66 x 5 box (one wave plus two nodes) every node of which carries the same populations is invariant under
    streaming: one step leaves every node with the post-collision state.  The populations are the equilibrium of a fixture
    state with every one of them scaled by a seeded factor in [0.9, 1.1]; all 48 states.  Bound: the twin in the kernels'
    format against the twin in the next wider one, times ORDER_FACTOR."""
    G = np.load(os.path.join(golden_dir, 'arith_sw_D2Q9.npz'))
    g = float(G['gravity'][k])
    R = _sw.DTYPE[precision]
    wide = tw.wider(R)
    desc, periodic, _ = _sw.box_desc((66, 5), 'AB', precision, gravity=g, visc=0.01)
    g = float(desc.gravity)            # as the module has it: the descriptor's member is a float
    gpu = BoxSim(backend, desc, periodic=periodic)
    rng = np.random.RandomState(11)
    omega = 1.0 / desc.tau
    try:
        _sw.start(gpu, _sw.seeded((66, 5)))
        worst = 0.0
        for n in range(len(G['h'])):
            h, v = np.array([G['h'][n]]), [np.array([G['v'][n, 0]]), np.array([G['v'][n, 1]])]
            f0 = (tw.sw_equilibrium(h, v, g, np.float64) * rng.uniform(0.9, 1.1, (9, 1))).astype(R)
            hh, vv = tw.lt.macro(tw.GRID, f0, False, R)
            want, _ = tw.sw_relax(f0, hh, vv, R(omega), R(0), None, False, g, R)
            if wide is not None:
                fw = f0.astype(wide)
                hw, vw = tw.lt.macro(tw.GRID, fw, False, wide)
                ref, _ = tw.sw_relax(fw, hw, vw, wide(omega), wide(0), None, False, g, wide)
                tol = ORDER_FACTOR * float(np.max(np.abs(want.astype(wide) - ref)))
            else:
                tol = ORDER_FACTOR * 16 * float(np.finfo(R).eps)
            full = np.full((9,) + gpu.shape, np.nan, dtype=R)
            gpu.real_view(full)[...] = f0[:, :, None]
            gpu.iteration = 0
            gpu.backend.set_iteration(0)
            gpu.set_dist(full, 0)
            gpu.step()
            got = gpu.real_view(gpu.get_dist())
            d = float(np.max(np.abs(got.astype(np.longdouble) - want[:, :, None].astype(np.longdouble))))
            worst = max(worst, d / tol if tol else (0.0 if d == 0 else np.inf))
            assert np.all(got == got[:, :1, :1])                 # every node the same
            assert d <= tol, (n, d, tol)
            assert abs(float(got[:, 0, 0].astype(np.float64).sum()) - float(f0.astype(np.float64).sum())) <= 16 * np.finfo(R).eps * 2
        print('largest difference / bound over the states: %.3f' % worst)
    finally:
        gpu.release()


# ---- twenty steps --------------------------------------------------------------------------------------------------------------

def test_twenty_steps_against_the_twin(backend):
    """Double precision, the Gaussian hump on 66 x 10, two-copy."""
    desc, periodic, _ = _sw.box_desc((66, 10), 'AB', 'double')
    twin, _ = run_against_twin(backend, desc, periodic, None, _sw.hump((66, 10)), 20)
    h = twin.real_view(twin.rho)
    assert h.max() < 1.39 and np.ptp(twin.real_view(twin.v[0])) > 1e-3         # the hump has started to collapse


# ---- walls ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('walls', ['full', 'half', 'slip'])
def test_walls_against_the_twin(backend, walls, pattern):
    """34 x 12, NTFullBBWall / NTHalfBBWall / NTSlip on the two y faces, x periodic; a seeded state that pushes against them."""
    desc, periodic, map_fn = _sw.box_desc((34, 12), pattern, 'double', walls=walls)
    twin, _ = run_against_twin(backend, desc, periodic, map_fn(desc), _sw.seeded((34, 12)), 8)
    if walls != 'full':         # (a full-way wall row holds the populations in flight through it)
        wet = twin.real_view(twin.current_dist())[:, 1:-1] if walls == 'slip' else twin.real_view(twin.current_dist())
        assert np.all(np.isfinite(wet))


# ---- forces -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('force', ['guo', 'edm'])
@pytest.mark.parametrize('precision', ['single', 'double'])
def test_constant_force_against_the_twin(backend, precision, force):
    desc, periodic, map_fn = _sw.box_desc((34, 12), 'AA', precision, walls='half', accel=(3e-5, -2e-5), force=force)
    run_against_twin(backend, desc, periodic, map_fn(desc), _sw.seeded((34, 12)), 6)


def test_time_dependent_force_against_the_twin(backend):
    """The acceleration is an argument of every launch (slf_module_set_body_force): a_x = 3e-5 sin(0.7 t)."""
    desc, periodic, _ = _sw.box_desc((34, 12), 'AB', 'double', accel=(0.0, 0.0))

    def set_force(step, gpu, twin):
        a = [3e-5 * np.sin(0.7 * step), 1e-5 * np.cos(0.7 * step)]
        gpu.backend.set_body_force(gpu.module, a)
        for i in range(2):
            twin.desc.accel[i] = a[i]
    run_against_twin(backend, desc, periodic, None, _sw.seeded((34, 12)), 6, per_step=set_force)


@pytest.mark.parametrize('force', ['guo', 'edm'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_acceleration_field_against_the_twin(backend, pattern, force):
    """A bed slope: a_x = c sin(2 pi gx / L) through the acceleration field, plus a uniform part."""
    size = (34, 12)
    y, x = np.mgrid[0:size[1], 0:size[0]].astype(np.float64)
    field = np.stack([4e-5 * np.sin(2.0 * np.pi * x / size[0]), np.zeros_like(x)])
    desc, periodic, map_fn = _sw.box_desc(size, pattern, 'double', walls='full', accel=(1e-5, 0.0), accel_field=True, force=force)
    run_against_twin(backend, desc, periodic, map_fn(desc), _sw.seeded(size), 6, accel_field=field)


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------

def _box_run(backend, steps, pattern, precision, fused=1, walls='half'):
    desc, periodic, map_fn = _sw.box_desc((34, 12), pattern, precision, walls=walls, fused=fused, accel=(2e-5, 1e-5))
    gpu = BoxSim(backend, desc, periodic=periodic, node_map=map_fn(desc))
    try:
        _sw.start(gpu, _sw.seeded((34, 12)))
        gpu.run(steps)
        rho, v = gpu.fetch_fields()
        return gpu.real_view(gpu.get_dist()).copy(), [gpu.real_view(a).copy() for a in [rho] + list(v)]
    finally:
        gpu.release()


@pytest.mark.parametrize('precision', ['single', 'double'])
def test_in_place_equals_two_copy(backend, precision):
    """After an even number of steps the in-place arrays hold what the two-copy ones hold; after an odd number the
    populations sit in the neighbours' opposite slots, so the fields are compared (as the free-energy test does)."""
    ab, fab = _box_run(backend, 10, 'AB', precision)
    aa, faa = _box_run(backend, 10, 'AA', precision)
    assert same(ab, aa) and all(same(a, b) for a, b in zip(fab, faa))
    _, fab = _box_run(backend, 11, 'AB', precision)
    _, faa = _box_run(backend, 11, 'AA', precision)
    assert all(same(a, b) for a, b in zip(fab, faa)) and np.ptp(fab[0][1:-1]) > 1e-3


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
def test_in_sweep_wrap_equals_ghost_layer_kernels(backend, precision, pattern):
    a, fa = _box_run(backend, 10, pattern, precision, fused=1)
    b, fb = _box_run(backend, 10, pattern, precision, fused=0)
    assert same(a, b) and all(same(x, y) for x, y in zip(fa, fb))


SPLIT_SIM = _sw.make_sim(walls='half', forces=[(1e-5, 2e-5), DynamicValue(2e-5 * S.gx, -1e-5 * S.gy)])


@pytest.fixture(scope='module')
def whole():
    out = {}
    for precision in ('single', 'double'):
        for pattern in ('AB', 'AA'):
            ctrl = _sw.run(SPLIT_SIM, _sw.config((34, 12), walls='half', pattern=pattern, precision=precision), 10)
            out[precision, pattern] = dict((w, merged(ctrl, w)) for w in ('dist', 'rho', 'v0', 'v1'))
    return out


@pytest.mark.parametrize('axis,cut', [(0, 16), (1, 5)], ids=['x', 'y'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
def test_one_subdomain_equals_two(whole, precision, pattern, axis, cut):
    ctrl = _sw.run(SPLIT_SIM, _sw.config((34, 12), walls='half', pattern=pattern, precision=precision), 10,
                   geo=_sw.strip_geometry(axis, cut))
    assert len(ctrl.runners) == 2
    for w in ('dist', 'rho', 'v0', 'v1'):
        got = merged(ctrl, w)
        assert np.all(np.isfinite(got)) and same(got, whole[precision, pattern][w]), w


def test_runner_equals_the_twin_behind_the_cpu_backend():
    """The whole host stack on the GPU against the same stack on the twin (tests/_sw_backend.py): double precision, walls,
    a time-dependent and a position-dependent force, 10 steps -- the kernels follow the twin's operation order, so the
    bound of twenty roundings per step is generous."""
    from sympy import sin
    sim = _sw.make_sim(walls='slip', forces=[DynamicValue(2e-5 * sin(0.3 * S.time), 0.0), DynamicValue(0.0, 1e-5 * sin(0.5 * S.gx))])
    cfg = _sw.config((34, 12), walls='slip')
    gpu = _sw.run(sim, cfg, 10)
    cpu = _sw.run(sim, cfg, 10, gpus=[0], backends='tests._sw_backend')
    for w in ('dist', 'rho', 'v0', 'v1'):
        a, b = merged(gpu, w), merged(cpu, w)
        assert _diff(a, b) <= ORDER_FACTOR * 10 * 20 * 0.5 * np.finfo(np.float64).eps * 2.0, w


# ---- physics -------------------------------------------------------------------------------------------------------------------------

def mass_bound(n, steps, dtype, hmax):
    """n nodes, `steps` steps: every population takes part in the density sum (Q - 1 additions), the relaxation and the
    rest population's difference once per step -- (Q + 2) roundings of half an ulp of values below max h per node and step
    (the bound of tests/test_gpu_fe.py::test_mass_and_order_parameter_are_conserved)."""
    return n * steps * (9 + 2) * 0.5 * float(np.finfo(dtype).eps) * hmax


def test_mass_is_conserved():
    """Single precision, periodic 32 x 8, 200 steps, a hump of amplitude 0.4: the drift of the total depth stays within
    n * steps * (Q + 2) * eps / 2 * max h.  The reference's rest population (its equilibrium sums to h + 2 h v^2) breaks this
    bound within a few steps: tests/test_sw_twin.py shows the growth on the twin."""
    class Mass(_sw.make_sim(fields='hump')):
        def after_step(self, runner):
            if self.iteration == 199:
                self.need_sync_flag = True
    ctrl = _sw.run(Mass, _sw.config((32, 8), pattern='AA', precision='single', gravity=0.05, visc=0.01), 200)
    h0, _ = _sw.global_fields((8, 32), 'hump')
    dist = merged(ctrl, 'dist').astype(np.float64)
    drift = abs(dist.sum() - h0.astype(np.float32).astype(np.float64).sum())
    bound = mass_bound(32 * 8, 200, np.float32, 1.4)
    print('mass drift %.3e, bound %.3e' % (drift, bound))
    assert drift <= bound
    # what the reference's rest population would have done by then, on the twin in the same format
    f = tw.model(32, 8, 0.05, 0.01, h0, 200, R=np.float32, rest=tw.sw_rest_reference)
    assert abs(float(f.astype(np.float64).sum()) - h0.sum()) > bound


def test_gravity_wave_period():
    """The 64 x 4 box, double precision, 600 steps, a 1 % cosine in h: the mode's period from zero crossings within 1 % of
    L / sqrt(g h0) (the twin is within 0.2 %)."""
    L, g = 64, 0.05
    mode = np.cos(2.0 * np.pi * np.arange(L) / L)
    signal = []

    class Wave(_sw.make_sim(fields='cosine')):
        def after_step(self, runner):
            self.need_fields_flag = self.need_sync_flag = True
            if self.iteration > 1:
                signal.append(float((np.asarray(self.rho, dtype=np.float64)[0] * mode).sum()))
    _sw.run(Wave, _sw.config((L, 4), pattern='AB', precision='double', gravity=g, visc=0.01), 600)
    period = tw.period_from_crossings(signal)
    theory = L / np.sqrt(g * 1.0)
    print('period %.3f, theory %.3f, relative difference %.2e' % (period, theory, period / theory - 1.0))
    assert abs(period / theory - 1.0) <= 0.01


# ---- refusals at module creation --------------------------------------------------------------------------------------------------

BASE = dict(lattice=hipabi.SLF_D2Q9, model=hipabi.SLF_BGK, precision=4, access_pattern=hipabi.SLF_AB, lat_nx=10, lat_ny=8,
            arr_nx=32, arr_ny=8, tau=0.8, visc=0.1, fluid_only=0, nt_type_mask=7, nt_misc_shift=3,
            type_kind=[0, 1, 2, 3, 4, 5, hipabi.SLF_NK_SLIP], equilibrium=hipabi.SLF_EQ_SHALLOW_WATER, gravity=0.05)
MODULE_REFUSALS = [
    (dict(model=hipabi.SLF_MRT), '--model=mrt'),
    (dict(model=hipabi.SLF_ELBM, entropy_tolerance=1e-6), '--model=elbm'),
    (dict(regularized=1), '--regularized'),
    (dict(subgrid=1, smagorinsky_const=0.1), '--subgrid'),
    (dict(incompressible=hipabi.SLF_DENSITY_ROUNDOFF), '--minimize_roundoff'),
    (dict(incompressible=hipabi.SLF_DENSITY_INCOMPRESSIBLE), '--incompressible'),
    (dict(node_addressing=hipabi.SLF_ADDR_INDIRECT, dist_stride=128), '--node_addressing=indirect'),
    (dict(type_kind=[0, 1, 2, 3, 4, hipabi.SLF_NK_EQUILIBRIUM_DENSITY]), 'carry a density or a velocity'),
    (dict(type_kind=[0, 1, 2, 3, 4, hipabi.SLF_NK_ZOUHE_VELOCITY]), 'carry a density or a velocity'),
    (dict(type_kind=[0, 1, 2, 3, 4, hipabi.SLF_NK_WALL_TMS]), 'NTWallTMS'),
    (dict(lattice=hipabi.SLF_D3Q19, lat_nz=6, arr_nz=6), 'D2Q9 only'),
    (dict(simtype=hipabi.SLF_SIM_FREE_ENERGY), 'free-energy'),
    (dict(gravity=0.0), 'gravity must be > 0'),
    (dict(equilibrium=2), 'equilibrium must be'),
]


@pytest.mark.parametrize('extra,word', MODULE_REFUSALS, ids=[w for _, w in MODULE_REFUSALS])
def test_refused_again_at_module_creation(backend, extra, word):
    served = backend.build(hipabi.make_desc(**BASE))
    assert served is not None
    with pytest.raises(backend.FatalError) as e:
        backend.build(hipabi.make_desc(**dict(BASE, **extra)))
    assert word in str(e.value)
    if word not in ('gravity must be > 0', 'equilibrium must be'):
        assert 'shallow water' in str(e.value)


# ---- the example ----------------------------------------------------------------------------------------------------------------------

def _run_example(args):
    """examples/fs_gaussian.py with a command line, in this process; returns the controller's runner fields."""
    from sailfish_amd import controller
    made = []
    orig = controller.LBSimulationController.run

    def run(self, *a, **kw):
        made.append(self)
        return orig(self, *a, **kw)
    argv = sys.argv
    controller.LBSimulationController.run = run
    sys.argv = [os.path.join(ROOT, 'examples', 'fs_gaussian.py')] + args
    try:
        runpy.run_path(sys.argv[0], run_name='__main__')
    finally:
        sys.argv = argv
        controller.LBSimulationController.run = orig
    return made[0]


@pytest.mark.parametrize('extra', [[], ['--bed_slope=0.002']], ids=['flat', 'bed_slope'])
def test_example_runs_and_the_hump_spreads(extra):
    """examples/fs_gaussian.py --periodic_x --periodic_y --max_iters=100 (62 x 62, visc 0.005, gravity 0.001, single
    precision): the water volume is kept to the bound of test_mass_is_conserved, the centre has dropped and the
    excess depth has moved outwards."""
    ctrl = _run_example(['--periodic_x', '--periodic_y', '--max_iters=100', '--quiet', '--every=100'] + extra)
    (r,) = ctrl.runners
    assert type(r._sim).__mro__[1].__name__ == 'LBFreeSurface' and r._desc.equilibrium == 1
    assert r._desc.accel_field == (1 if extra else 0)
    h = np.asarray(r._sim.rho, dtype=np.float64)
    assert h.shape == (62, 62)
    h0, _ = _sw.hump((62, 62))
    dist = merged(ctrl, 'dist').astype(np.float64)
    drift = abs(dist.sum() - h0.astype(np.float32).astype(np.float64).sum())
    bound = mass_bound(62 * 62, 100, np.float32, 1.4)
    print('mass drift %.3e, bound %.3e' % (drift, bound))
    assert drift <= bound
    assert h[31, 31] < h0[31, 31] - 0.05                                   # the centre depth has dropped
    # The ring: at sqrt(g h) = 0.032 .. 0.037 nodes per step the front has moved some 3.5 nodes in 100 steps, less than the
    # hump's width of 62 / 12, so the crest has not left the centre yet; what has grown is the radius of the excess depth,
    # sum (h - 1) r / sum (h - 1) -- by more than a node, and to what the twin gives (the stored fields are those of step 99)
    y, x = np.mgrid[0:62, 0:62]
    r = np.hypot(x - 31.0, y - 31.0)

    def radius(depth):
        return float(((depth - 1.0) * r).sum() / (depth - 1.0).sum())
    print('centre depth %.4f (from %.4f), radius of the excess depth %.3f (from %.3f)' % (h[31, 31], h0[31, 31], radius(h), radius(h0)))
    assert radius(h) > radius(h0) + 1.0
    if not extra:
        ht = tw.model(62, 62, 0.001, 0.005, h0, 99, R=np.float32).astype(np.float64).sum(axis=0)
        assert abs(radius(h) - radius(ht)) <= 1e-3 and abs(h[31, 31] - ht[31, 31]) <= 1e-4
