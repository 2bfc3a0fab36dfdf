"""Body forces that depend on position on the GPU: the ACCF instantiations of the per-node sweep (csrc/slf_kernels.hip)
against the numpy twin (tests/_accf_twin.py) and the CPU oracle, bit for bit; decompositions against the undivided run; the
four-rolls mill and the Taylor-Green vortices against their closed-form solutions; the refusals of the C ABI."""
import ctypes
import math

import numpy as np
import pytest

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish_amd import geo as geo_mod
from sailfish_amd import hipabi, sym
from sailfish_amd.box import BoxSim
from sailfish_amd.lb_base import LBForcedSim
from sailfish_amd.lb_single import LBFluidSim
from sailfish_amd.node_type import DynamicValue
from sailfish_amd.subdomain import Subdomain3D
from sailfish_amd.sym import S
from tests import _accf, _lat, _open_sims
from tests._accf_twin import AccfTwinBox, linear_field
from tests._oracle_box import OracleBox

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. parity with the twin --------------------------------------------------------------------------------------------------
# partial waves, arr_nx != lat_nx (70 + 2 -> 96, 130 + 2 -> 160, 34 + 2 -> 64), more than one wave per row
BOXES = [('D2Q9', (70, 9)), ('D2Q9', (130, 5)), ('D3Q19', (34, 5, 4)), ('D3Q19', (70, 4, 3))]
UNIFORM = [0.7e-5, -0.4e-5, 0.9e-5]       # the uniform part, so that the sum cp.accel + field is exercised as well


@pytest.mark.parametrize('force', ['guo', 'edm'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name,size', BOXES, ids=['%s-%s' % (n, 'x'.join(map(str, s))) for n, s in BOXES])
def test_parity_with_the_twin(backend, name, size, precision, pattern, force):
    """Six steps, populations and rho / v after every one; fully periodic through the in-sweep wrap and through the
    ghost-layer kernels, full-way and half-way walls on the two y faces.  The field is linear in x, y, z with distinct
    coefficients in every component; the padding and ghost entries of the uploaded array are NaN."""
    grid = _accf.GRIDS[name]
    dim = grid.dim
    field = linear_field(size, dim)
    for walls, fused in ((None, 1), (None, 0), ('full', 1), ('half', 1)):
        uniform = UNIFORM[:dim] if walls != 'full' else None
        desc, periodic, map_fn = _accf.box_desc(grid, size, pattern, precision, force, walls, fused, accel=uniform,
                                                accel_field=True)
        nmap = None if map_fn is None else map_fn(desc)
        twin = _accf.start(AccfTwinBox(desc, periodic, nmap, accel_field=field), size, dim)
        gpu = BoxSim(backend, desc, periodic=periodic, node_map=nmap, accel_field=field, accel_field_fill=np.nan)
        try:
            assert np.isnan(gpu.accel_field).sum() == gpu.accel_field.size - field.size
            assert same(gpu.accel_field, twin.accel_field)
            _accf.start(gpu, size, dim)
            for step in range(6):
                twin.step(save_macro=True)
                gpu.step(save_macro=True)
                what = (walls, fused, step)
                assert same(gpu.real_view(gpu.get_dist()), twin.real_view(twin.current_dist())), what
                rho, v = gpu.fetch_fields()
                assert same(gpu.real_view(rho), twin.real_view(twin.rho)), what
                for k in range(dim):
                    assert same(gpu.real_view(v[k]), twin.real_view(twin.v[k])), what
            assert np.all(np.isfinite(gpu.real_view(gpu.get_dist())))
        finally:
            gpu.release()


# ---- 2. a uniform field is a constant force -------------------------------------------------------------------------------------

class _UniformValue(object):
    """Stands where a DynamicValue of position stands (a sympy expression that does not vary simplifies to a constant):
    the same value at every node."""

    def __init__(self, value):
        self.value = np.asarray(value, dtype=np.float64)

    def evaluate(self, coords, iteration, dt):
        return np.tile(self.value, (len(coords[0]), 1))


def forced_pair(base, accel):
    """(simulation with the constant acceleration, the same with the acceleration as a uniform field)"""
    class Constant(base, LBForcedSim):
        def __init__(self, config):
            super(Constant, self).__init__(config)
            self.add_body_force(tuple(accel))

    class Field(base, LBForcedSim):
        def __init__(self, config):
            super(Field, self).__init__(config)
            self._field_forces.append(_UniformValue(accel))
    return Constant, Field


def _cavity():
    from examples.ldc_2d import CavitySim
    return CavitySim


SETUPS = {
    # full-way walls, regularized-velocity inlet, do-nothing outlet (a boundary condition in place, plain fluid two-copy)
    'open-channel': (lambda: _open_sims.OpenChannelSim, 2, dict(lat_nx=40, lat_ny=12, visc=0.05), (1e-5, -2e-5)),
    'open-duct': (lambda: _open_sims.OpenDuctSim, 3, dict(lat_nx=34, lat_ny=8, lat_nz=10, visc=0.05), (1e-5, -2e-5, 3e-5)),
    # full-slip walls: the instantiation for the module's highest boundary-condition level
    'slip-channel': (lambda: _open_sims.framed_sim(2, (0, 1), walls='slip', inlet=None, outlet=None), 2,
                     dict(lat_nx=40, lat_ny=12, visc=0.05), (1e-5, -2e-5)),
    'cavity': (_cavity, 2, dict(lat_nx=40, lat_ny=24, visc=0.05), (1e-5, -2e-5)),
}


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('model', ['bgk', 'mrt'])
@pytest.mark.parametrize('setup', sorted(SETUPS))
def test_uniform_field_equals_constant_force(setup, model, precision, pattern):
    base, dim, cfg, accel = SETUPS[setup]
    base = base()
    constant, field = forced_pair(base, accel)
    geo = geo_mod.LBGeometry2D if dim == 2 else geo_mod.LBGeometry3D
    cfg = dict(cfg, model=model, precision=precision, access_pattern=pattern)
    cfg.update(getattr(base, 'periodic_cfg', {}))
    a = _lat.run_gpu(constant, cfg, 10, geo)
    b = _lat.run_gpu(field, cfg, 10, geo)
    da, db = a.runners[0]._desc, b.runners[0]._desc
    assert (da.accel_field, da.has_force, db.accel_field, db.has_force) == (0, 1, 1, 1)
    assert list(db.accel) == [0.0, 0.0, 0.0] and list(da.accel)[:dim] == list(accel)
    fa, fb = _lat.merged(a, 'dist'), _lat.merged(b, 'dist')
    wet = a.runners[0]._subdomain.fluid_map(wet=True)
    assert wet.any() and np.all(np.isfinite(fa[:, wet]))
    assert np.array_equal(fa[:, wet], fb[:, wet])
    for what in ['rho'] + ['v%d' % k for k in range(dim)]:
        assert np.array_equal(_lat.merged(a, what)[wet], _lat.merged(b, what)[wet]), what


# ---- 3. MRT with a non-uniform field, composed from constant-force oracle steps -----------------------------------------------------

BANDS = [(1.1e-5, -2.3e-5, 0.7e-5), (-3.1e-5, 0.9e-5, 1.9e-5), (0.4e-5, 2.7e-5, -1.3e-5)]


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name,size', [('D2Q9', (70, 9)), ('D3Q19', (34, 5, 6))])
def test_mrt_is_composed_of_constant_force_steps(backend, name, size, precision):
    """The collision is local: with the field constant in three bands along y (z in 3-D), every node of a band comes out of
    the module with the field as it comes out of the oracle's constant-force module with that band's value -- the
    populations of one in-place even step (stored to the own node) and the rho / v output of one two-copy step."""
    grid = _accf.GRIDS[name]
    dim = grid.dim
    shape = tuple(reversed(size))
    n = shape[0]
    band = np.minimum(np.arange(n) * 3 // n, 2)                          # band of a layer of the slowest axis
    layers = band.reshape((n,) + (1,) * (dim - 1))
    field = np.stack([np.broadcast_to(np.array([b[k] for b in BANDS])[layers], shape) for k in range(dim)])
    rng = np.random.RandomState(3)
    for pattern in ('AA', 'AB'):
        desc, periodic, _ = _accf.box_desc(grid, size, pattern, precision, 'guo', accel_field=True, model='mrt')
        gpu = BoxSim(backend, desc, periodic=periodic, accel_field=field, accel_field_fill=np.nan)
        try:
            w = np.array([float(x) for x in grid.weights]).reshape((grid.Q,) + (1,) * 3)
            start = (w * (1.0 + 0.05 * rng.rand(*((grid.Q,) + gpu.shape)))).astype(gpu.dtype)      # not an equilibrium
            gpu.initial_conditions()
            gpu.set_dist(start)
            gpu.step(save_macro=True)
            got = gpu.real_view(gpu.get_dist())
            rho, v = gpu.fetch_fields()
            got_fields = [gpu.real_view(rho)] + [gpu.real_view(c) for c in v]
            for b, accel in enumerate(BANDS):
                d_o, _, _ = _accf.box_desc(grid, size, pattern, precision, 'guo', accel=accel[:dim], model='mrt')
                o = OracleBox(d_o, periodic)
                o.initial_conditions()
                o.dist[0][...] = start
                o.step(save_macro=True)
                sel = band == b
                if pattern == 'AA':
                    assert np.array_equal(got[:, sel], o.real_view(o.current_dist())[:, sel]), (pattern, b)
                want_fields = [o.real_view(o.rho)] + [o.real_view(o.v[k]) for k in range(dim)]
                for g, want in zip(got_fields, want_fields):
                    assert np.array_equal(g[sel], want[sel]), (pattern, b)
            assert np.all(np.isfinite(got))
        finally:
            gpu.release()


# ---- 4. decompositions ----------------------------------------------------------------------------------------------------------

def _mill():
    from examples.four_rolls_mill import FourRollsMill
    return FourRollsMill


MILL = dict(lat_nx=64, lat_ny=32, visc=0.05, max_v=0.02, lambda_x=1, lambda_y=1, err_every=10 ** 6)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_mill_decompositions_equal_the_undivided_run(pattern):
    cfg = dict(MILL, access_pattern=pattern, precision='single')
    one = _lat.run_gpu(_mill(), cfg, 40, geo_mod.EqualSubdomainsGeometry2D)
    assert len(one.runners) == 1 and one.runners[0]._desc.accel_field == 1
    whole = [_lat.merged(one, w) for w in ('dist', 'rho', 'v0', 'v1')]
    assert np.all(np.isfinite(whole[0])) and np.ptp(whole[2]) > 0
    for axis in ('x', 'y'):
        two = _lat.run_gpu(_mill(), dict(cfg, subdomains=2, conn_axis=axis), 40, geo_mod.EqualSubdomainsGeometry2D)
        assert len(two.runners) == 2
        for w, want in zip(('dist', 'rho', 'v0', 'v1'), whole):
            assert np.array_equal(_lat.merged(two, w), want), (axis, w)


FIELD3 = DynamicValue(1.0e-5 + 2.3e-6 * S.gx - 1.1e-6 * S.gy, -0.7e-5 + 0.9e-6 * S.gz + 1.7e-6 * S.gx,
                      0.45e-5 - 1.3e-6 * S.gy + 0.6e-6 * S.gz)


class _Box3(Subdomain3D):
    def boundary_conditions(self, hx, hy, hz):
        pass

    def initial_conditions(self, sim, hx, hy, hz):
        rho, v = _lat.global_fields((self.gz, self.gy, self.gx))
        where = (hz, hy, hx)
        sim.rho[:] = rho[where]
        for c, a in zip((sim.vx, sim.vy, sim.vz), v):
            c[:] = a[where]


class _Sim3(LBFluidSim, LBForcedSim):
    subdomain = _Box3

    def __init__(self, config):
        super(_Sim3, self).__init__(config)
        self.add_body_force(FIELD3)
        self.add_body_force((2e-6, 0.0, -1e-6))


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_3d_box_split_along_x_equals_the_undivided_run(pattern):
    cfg = dict(lat_nx=34, lat_ny=6, lat_nz=6, periodic_x=True, periodic_y=True, periodic_z=True, visc=0.05,
               access_pattern=pattern, precision='single')
    one = _lat.run_gpu(_Sim3, cfg, 40, geo_mod.LBGeometry3D)
    two = _lat.run_gpu(_Sim3, dict(cfg, subdomains=2, conn_axis='x'), 40, geo_mod.EqualSubdomainsGeometry3D)
    assert len(one.runners) == 1 and len(two.runners) == 2
    assert np.all(np.isfinite(_lat.merged(one, 'dist')))
    for w in ('dist', 'rho', 'v0', 'v1', 'v2'):
        assert np.array_equal(_lat.merged(two, w), _lat.merged(one, w)), w


# ---- 5. physics -----------------------------------------------------------------------------------------------------------------
# 64 x 64, visc = 0.1, max_v = 0.02 (Mach 0.035), 500 steps: the free vortices decay by exp(-visc k^2 t) = exp(-0.1 x
# 2 (2 pi / 64)^2 x 499) = 0.382 of their amplitude.  Relative L2 velocity errors of the double-precision twin
# (tests/_accf_twin.py) on this set-up, measured on the CPU, fields of the last step against the solution at t = 499:
TWIN_MILL_ERROR = 8.435671e-04       # forced (the mill), against the steady solution
TWIN_FREE_ERROR = 1.243560e-03       # unforced, against the decayed solution (6.85e-4 against the solution at t = 500)
PHYSICS = dict(lat_nx=64, lat_ny=64, visc=0.1, max_v=0.02, lambda_x=1, lambda_y=1, err_every=10 ** 6)
STEPS = 500


def _velocity_error(ctrl, sim_cls, t):
    cfg = ctrl.runners[0].config
    hy, hx = np.mgrid[0:cfg.lat_ny, 0:cfg.lat_nx].astype(np.float64)
    mach = cfg.max_v / math.sqrt(1.0 / 3.0)
    _, ref_vx, ref_vy = sim_cls.subdomain.solution(cfg, hx, hy, cfg.lat_nx, cfg.lat_ny, t, mach)
    vx, vy = [_lat.merged(ctrl, w).astype(np.float64) for w in ('v0', 'v1')]
    return math.sqrt(((ref_vx - vx) ** 2 + (ref_vy - vy) ** 2).sum() / (ref_vx ** 2 + ref_vy ** 2).sum())


@pytest.mark.parametrize('precision', ['single', 'double'])
def test_mill_stays_steady_and_free_vortices_decay(precision):
    """The factor two covers single-precision round-off, which is orders below the discretisation error at this Mach
    number."""
    from examples.taylor_green_2d import TaylorGreenSim
    k_sq = 2.0 * (2.0 * math.pi / 64) ** 2
    assert math.exp(-PHYSICS['visc'] * k_sq * (STEPS - 1)) < 0.5
    cfg = dict(PHYSICS, precision=precision)
    mill = _lat.run_gpu(_mill(), cfg, STEPS, geo_mod.EqualSubdomainsGeometry2D)
    err = _velocity_error(mill, _mill(), 0)                               # steady: the state at t = 0
    print('four rolls mill, %s: relative velocity error %.6e (twin %.6e)' % (precision, err, TWIN_MILL_ERROR))
    free = _lat.run_gpu(TaylorGreenSim, cfg, STEPS, geo_mod.EqualSubdomainsGeometry2D)
    err_free = _velocity_error(free, TaylorGreenSim, STEPS - 1)          # the fields are those the last step started from
    print('taylor green, %s: relative velocity error %.6e (twin %.6e)' % (precision, err_free, TWIN_FREE_ERROR))
    vmax = np.abs(_lat.merged(free, 'v0')).max()
    assert 0.3 * PHYSICS['max_v'] / math.sqrt(2.0) < vmax < 0.5 * PHYSICS['max_v'] / math.sqrt(2.0)       # it did decay
    assert err <= 2.0 * TWIN_MILL_ERROR
    assert err_free <= 2.0 * TWIN_FREE_ERROR


# ---- 6. refusals at the C ABI ------------------------------------------------------------------------------------------------------

def test_c_abi_refuses_a_field_without_the_flag_and_a_launch_without_a_field(backend):
    grid, size = sym.D3Q19, (34, 5, 4)
    lib = backend._lib
    # a module created without accel_field takes no field
    plain, periodic, _ = _accf.box_desc(grid, size, 'AB', 'single', 'guo', accel=[1e-5, 0.0, 0.0])
    s = BoxSim(backend, plain, periodic=periodic)
    try:
        rc = lib.slf_module_set_accel_field(s.module.handle, ctypes.c_void_p(s.gpu_rho))
        assert rc == 1 and b'accel_field' in lib.slf_last_error()             # SLF_ERR_INVALID
    finally:
        s.release()
    # a module created with it does not launch before one is set -- and launches nothing
    desc, periodic, _ = _accf.box_desc(grid, size, 'AB', 'single', 'guo', accel_field=True)
    s = BoxSim(backend, desc, periodic=periodic)
    try:
        _accf.start(s, size, 3)
        before = [s.get_dist(0), s.get_dist(1)]
        k = s.k_sweep[0][0]
        rc = lib.slf_kernel_launch(k.handle, None, s.stream.handle)
        assert rc == 1 and b'slf_module_set_accel_field' in lib.slf_last_error()
        assert lib.slf_module_set_accel_field(s.module.handle, None) == 1      # NULL is no field either
        s.sync()
        assert same(s.get_dist(0), before[0]) and same(s.get_dist(1), before[1])
        # with a field the same kernel object launches
        field = np.zeros((3,) + s.shape, dtype=s.dtype)
        addr = backend.alloc_buf(like=field)
        backend.set_accel_field(s.module, addr)
        assert lib.slf_kernel_launch(k.handle, None, s.stream.handle) == 0
        s.sync()
        assert not same(s.get_dist(1), before[1])
        backend.free_buf(addr)
    finally:
        s.release()
    assert s.module.block_size <= 512
