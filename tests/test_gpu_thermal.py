"""Thermal flows on the GPU (csrc/slf_thermal.hip behind slf_thermal_*; lb_thermal.LBThermalFluidSim with
ThermalSubdomainRunner) against the numpy twin (tests/_thermal_twin.py), bit for bit; repeatability, step plans, restore;
conduction, an advected wave and the Rayleigh-Benard onset within the bounds measured with the twin; the refusals of the
C ABI."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from sailfish_amd import geo as geo_mod
from sailfish_amd import hipabi, sym
from tests import _accf, _lat, _thermal
from tests.test_thermal_twin import WAVE_L2, WAVE_RATE, WAVE_SPEED, WAVE_SPEED_F32

pytestmark = pytest.mark.gpu

TAU_T, T_REF = 0.8, 0.5
B = [0.4e-3, 1.1e-3, -0.7e-3]          # three distinct components, so that no axis mix-up can hide


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. parity with the twin --------------------------------------------------------------------------------------------------
# The full cross of the issue: three shapes -- rows that cross a wave boundary and are no multiple of 64 (70), or span three
# waves (130) -- x f32 / f64 x AB / AA x BGK / MRT x {no map, map} x {periodic on x only, on every axis, on none}.  The last
# two factors are the six geometry kinds of tests/_thermal.py (the 3-D channel with a map is periodic on x and z).
SHAPES = [(70, 9), (130, 9), (70, 6, 5)]
PARITY = list(itertools.product(SHAPES, ['open_x', 'periodic', 'open', 'channel', 'block', 'box'], ['single', 'double'],
                                ['AB', 'AA'], ['bgk', 'mrt']))
assert len(PARITY) == 144


@pytest.mark.parametrize('size,kind,precision,pattern,model', PARITY,
                         ids=['%s-%s-%s-%s-%s' % ('x'.join(map(str, c[0])), c[1], c[2], c[3], c[4]) for c in PARITY])
def test_parity_with_the_twin(backend, size, kind, precision, pattern, model):
    """T, both copies of the populations, the field, rho and v after the init launch and after 1, 2 and 7 steps, with NaN in
    every entry no kernel may read or write (ghost layers, padding, the populations and T of dry nodes).  BGK: the whole
    state.  MRT: the twin's fluid step is BGK only (tests/_accf_twin.py), so the twin takes rho and v of every step from the
    device and the thermal arithmetic is held against it bit for bit; the MRT sweep itself is the unchanged ACCF sweep
    (tests/test_gpu_accel_field.py)."""
    dim = len(size)
    desc, periodic, nmap, wall_t = _thermal.geometry(kind, size, pattern, precision, model)
    d_twin = desc if model == 'bgk' else _thermal.geometry(kind, size, pattern, precision)[0]
    T0 = _thermal.start_temperature(size)
    twin = _thermal.start(_thermal.twin_box(d_twin, periodic, nmap, T0, wall_t, TAU_T, T_REF, B[:dim]), kind, size)
    gpu = _thermal.BoxWithThermal(backend, desc, periodic, nmap, T0, wall_t, TAU_T, T_REF, B[:dim])
    try:
        _thermal.start(gpu, kind, size)
        wet = twin.t.wet
        n_real = int(np.prod(size))

        def compare(step):
            for c in (0, 1):
                assert same(gpu.populations(c), twin.t.g[c]), (step, c)
            T = gpu.temperature_array()
            assert same(T, twin.t.T), step
            field = gpu.field()
            assert same(field, twin.accel_field), step
            assert np.isnan(field).sum() == field.size - dim * n_real          # ghost and padding entries untouched
            assert np.isfinite(T[wet & ~np.isnan(twin.t.T)]).all()
            if model == 'bgk':
                assert same(gpu.box.real_view(gpu.box.get_dist()), twin.real_view(twin.current_dist())), step
                rho, v = gpu.box.fetch_fields()
                assert same(gpu.box.real_view(rho), twin.real_view(twin.rho)), step
                for k in range(dim):
                    assert same(gpu.box.real_view(v[k]), twin.real_view(twin.v[k])), step

        compare(0)
        assert np.isnan(twin.t.g[1]).all()                                      # the init launch writes copy 0 only
        for step in range(1, 8):
            gpu.box.step(save_macro=True)
            if model == 'bgk':
                super(type(twin), twin).step(save_macro=True)
            else:
                rho, v = gpu.box.fetch_fields()
                twin.rho[...] = rho
                for k in range(dim):
                    twin.v[k][...] = v[k]
            gpu.lattice_step()
            twin.lattice_step()
            if step in (1, 2, 7):
                compare(step)
        # dry nodes: populations never written; the poison of wall_temperature was never read and is still there
        if nmap is not None:
            dry = ~wet
            assert np.isnan(twin.t.g[0][:, dry]).all() and np.isnan(gpu.populations(0)[:, dry]).all()
        assert same(gpu.wall_temperature_array(), gpu.wall_t)
        assert np.abs(twin.accel_field[~np.isnan(twin.accel_field)]).max() > 1e-5          # the buoyancy is there
    finally:
        gpu.release()


@pytest.mark.parametrize('dim,precision', [(2, 'single'), (2, 'double'), (3, 'single'), (3, 'double')])
def test_open_faces_bounce_back(backend, dim, precision):
    """No node map and no periodic axis: a pull from beyond the real nodes takes the node's own opposite population, and
    wall_temperature is not read (its ghost entries hold a finite poison).  The thermal launch alone, on a fixed seeded
    velocity, 7 steps, against the twin bit for bit; heat is conserved."""
    from sailfish_amd.box import make_box_desc
    size = (70, 9) if dim == 2 else (70, 6, 5)
    desc = make_box_desc(_thermal.GRIDS[dim], size, precision=precision, access_pattern='AB', accel_field=True)
    T0 = _thermal.start_temperature(size)
    rho, v = _accf.start_fields(size, dim)
    periodic = (False, False, False)
    twin = _thermal.twin_box(desc, periodic, None, T0, None, TAU_T, T_REF, B[:dim])
    gpu = _thermal.BoxWithThermal(backend, desc, periodic, None, T0, None, TAU_T, T_REF, B[:dim])
    try:
        twin.set_fields(rho, v)
        twin.t.init(twin.v)
        gpu.set_fields(rho, v)
        gpu.lat.init(gpu.box.gpu_map, gpu.gpu_T, gpu.box.gpu_v, gpu.box.stream)
        for _ in range(7):
            twin.lattice_step()
            gpu.lattice_step()
        for c in (0, 1):
            assert same(gpu.populations(c), twin.t.g[c])
        assert same(gpu.temperature_array(), twin.t.T) and same(gpu.field(), twin.accel_field)
        assert abs(gpu.temperature().astype(np.float64).sum() - T0.sum()) < 1e-4 * T0.sum()
    finally:
        gpu.release()


# ---- 2. the runner: repeatability, step plans, restore -----------------------------------------------------------------------------

def thermal_sim(dim, size, kind):
    from sailfish_amd.lb_thermal import LBThermalFluidSim
    from sailfish_amd.node_type import NTFullBBWall
    from sailfish_amd.subdomain import Subdomain2D, Subdomain3D
    base = Subdomain2D if dim == 2 else Subdomain3D
    start = _accf.start_fields(size, dim)
    T0 = _thermal.start_temperature(size)

    class Layer(base):
        def boundary_conditions(self, *h):
            if kind == 'channel':
                self.set_node((h[1] == 0) | (h[1] == self.gy - 1), NTFullBBWall)

        def initial_conditions(self, sim, *h):
            where = tuple(reversed(h))
            sim.rho[:] = start[0][where]
            for c, a in zip(sim.v, start[1]):
                c[:] = a[where]
            sim.T[:] = T0[where]
            if kind == 'channel':
                sim.wall_temperature[h[1] == 0] = 1.0
                sim.wall_temperature[h[1] == self.gy - 1] = 0.0

    class Sim(LBThermalFluidSim):
        subdomain = Layer

        def __init__(self, config):
            super(Sim, self).__init__(config)
            self.set_buoyancy(B[:dim], t_ref=T_REF)
            self.add_body_force(tuple([1e-5, 0.0, 0.0][:dim]))

    return Sim


def run_thermal(dim, kind, pattern, precision, model, steps=12, **over):
    size = (70, 9) if dim == 2 else (70, 6, 5)
    cfg = dict(lat_nx=size[0], lat_ny=size[1], periodic_x=True, periodic_y=kind != 'channel', access_pattern=pattern,
               precision=precision, model=model, visc=0.05, thermal_diffusivity=0.1)
    if dim == 3:
        cfg.update(lat_nz=size[2], periodic_z=True)
    cfg.update(over)
    geo = geo_mod.LBGeometry2D if dim == 2 else geo_mod.LBGeometry3D
    return _lat.run_gpu(thermal_sim(dim, size, kind), cfg, steps, geo)


def state(ctrl):
    r = ctrl.runners[0]
    r.backend.from_buf(r._gpu_accel_field)
    return [r._debug_get_dist(), r.thermal_populations(), np.array(r._host_accel_field), r._sim.T, r._sim.rho] + list(r._sim.v)


CASES = [(2, 'channel', 'AB', 'single', 'bgk'), (2, 'periodic', 'AA', 'double', 'mrt'), (3, 'channel', 'AA', 'single', 'bgk'),
         (3, 'periodic', 'AB', 'double', 'mrt')]


@pytest.mark.parametrize('dim,kind,pattern,precision,model', CASES)
def test_two_runs_are_bit_identical_and_step_plans_change_nothing(dim, kind, pattern, precision, model):
    a = run_thermal(dim, kind, pattern, precision, model)
    r = a.runners[0]
    assert type(r).__name__ == 'ThermalSubdomainRunner' and r._desc.accel_field == 1
    b = run_thermal(dim, kind, pattern, precision, model)
    c = run_thermal(dim, kind, pattern, precision, model, hip_step_plans=False)
    assert a.runners[0]._step_plans.plans and not c.runners[0]._step_plans.plans
    for x, y, z in zip(state(a), state(b), state(c)):
        assert same(x, y) and same(x, z)
    T = np.array(r._sim.T)
    wet = np.ones(T.shape, dtype=bool)
    if kind == 'channel':
        wet[..., 0, :] = wet[..., -1, :] = False
    assert np.isfinite(T[wet]).all() and np.ptp(T[wet]) > 0.01
    assert np.abs(state(a)[2]).max() > 1e-5                                      # the buoyancy reached the field


@pytest.mark.parametrize('dim,kind,pattern,precision,model', CASES)
def test_restored_run_equals_the_straight_run(dim, kind, pattern, precision, model, tmp_path):
    straight = run_thermal(dim, kind, pattern, precision, model)
    ck = str(tmp_path / 'ck')
    run_thermal(dim, kind, pattern, precision, model, steps=7, checkpoint_file=ck, final_checkpoint=True)
    cp = [f for f in os.listdir(str(tmp_path)) if f.startswith('ck') and f.endswith('.cpoint.npz')]
    assert len(cp) == 1
    restored = run_thermal(dim, kind, pattern, precision, model,
                           restore_from=os.path.join(str(tmp_path), cp[0][:-len('.0.cpoint.npz')]))
    assert restored.runners[0]._sim.iteration == 12
    for x, y in zip(state(straight), state(restored)):
        assert same(x, y)


# ---- 3. physics: the cases of tests/test_thermal_twin.py on the device, within the bounds measured there --------------------------

def device_box(backend, made):
    def make(*args):
        made.append(_thermal.BoxWithThermal(backend, *args))
        return made[-1]
    return make


@pytest.fixture
def make(backend):
    made = []
    yield device_box(backend, made)
    for sim in made:
        sim.release()


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('tau_t,H,steps', _thermal.CONDUCTION)
def test_conduction_profile(make, precision, tau_t, H, steps):
    """The straight line through the link mid-points to 100 eps of the precision (the twin, which the device equals bit for
    bit: 40.5 / 60 / 3 eps in double, 22 / 41 / 1.5 eps in single precision)."""
    dev = _thermal.conduction(make, precision, tau_t, H, steps)
    print('conduction, %s, tau_T = %g, H = %d: %.1f eps' % (precision, tau_t, H, dev))
    assert dev <= 100.0


@pytest.mark.parametrize('precision', ['single', 'double'])
def test_advected_sine_wave(make, precision):
    """Twice the twin's error (tests/test_thermal_twin.py) on every figure, in both precisions: the relative L2 error of the
    perturbation against 0.1 exp(-kappa k^2 t) sin(k (x - u t)), the fitted decay rate, the fitted phase speed.  L2 error and
    decay rate are bounded by the double-precision twin's, as the issue states.  So is the phase speed in double precision.
    In single precision the phase speed departs from '2 x the f64 error': the double twin's 1.8e-8 is below what the format
    resolves (T = 0.5 +- 0.1 rounds to 3e-8 per node and step), so the bound there is twice the SINGLE-precision twin's own
    error, 1.02e-6 (2e-5 nodes of travel after 400 steps), measured on the CPU and pinned in WAVE_SPEED_F32."""
    l2, rate, speed = _thermal.advected_wave(make, precision)
    print('advected wave, %s: relative L2 error %.4e, decay rate error %.4e, phase speed error %.4e' % (precision, l2, rate, speed))
    assert l2 <= 2.0 * WAVE_L2
    assert abs(rate) <= 2.0 * WAVE_RATE
    assert abs(speed) <= 2.0 * (WAVE_SPEED if precision == 'double' else WAVE_SPEED_F32)


@pytest.mark.parametrize('precision', ['single', 'double'])
def test_rayleigh_benard_onset(make, precision):
    """Kinetic energy at the end >= 2 x its mid-run value at Ra = 5000, <= 1/2 x at Ra = 800, peak speed below 0.1 (the
    double-precision twin: 76.6 and 0.112, peak 3.7e-3)."""
    growth, peak_above = _thermal.rayleigh_benard(make, precision, _thermal.RB['above'])
    decay, peak_below = _thermal.rayleigh_benard(make, precision, _thermal.RB['below'])
    print('Rayleigh-Benard, %s: KE ratio %.3f at Ra = 5000 (peak %.3e), %.4f at Ra = 800 (peak %.3e)'
          % (precision, growth, peak_above, decay, peak_below))
    assert growth >= 2.0 and decay <= 0.5
    assert max(peak_above, peak_below) < 0.1


# ---- 4. refusals at the C ABI -----------------------------------------------------------------------------------------------------

def test_c_abi_refuses_what_the_bind_program_lists(backend):
    lib = backend._lib
    grid, size = sym.D3Q19, (16, 5, 4)
    P = ctypes.c_void_p
    from sailfish_amd.box import BoxSim, make_box_desc
    params = backend.thermal_params(1.25, 0.5, [0.0, 1e-3, 0.0], [True, True, True])
    ref = ctypes.byref(params)

    def step(s, p, *ptrs):
        return lib.slf_thermal_step(s.module.handle, p, *(list(ptrs) + [s.stream.handle]))

    plain, periodic, _ = _accf.box_desc(grid, size, 'AB', 'single', 'guo', accel=[1e-5, 0.0, 0.0])
    s = BoxSim(backend, plain, periodic=periodic)
    try:
        a, c = P(s.gpu_rho), P(s.gpu_v[0])
        assert step(s, ref, None, a, c, a, a, a, a, a) == 1
        assert b'slf_thermal_step' in lib.slf_last_error() and b'accel_field' in lib.slf_last_error()
    finally:
        s.release()
    desc, periodic, _ = _accf.box_desc(grid, size, 'AB', 'single', 'guo', accel_field=True)
    s = BoxSim(backend, desc, periodic=periodic)                         # created with the flag, no field set yet
    try:
        a, c = P(s.gpu_rho), P(s.gpu_v[0])
        assert step(s, ref, None, a, c, a, a, a, a, a) == 1 and b'slf_module_set_accel_field' in lib.slf_last_error()
        field = np.zeros((3,) + s.shape, dtype=s.dtype)
        addr = backend.alloc_buf(like=field)
        backend.set_accel_field(s.module, addr)
        assert step(s, None, None, a, c, a, a, a, a, a) == 1 and b'params is NULL' in lib.slf_last_error()
        assert step(s, ref, None, a, a, a, a, a, a, a) == 1 and b'g_src == g_dst' in lib.slf_last_error()
        assert step(s, ref, None, None, c, a, a, a, a, a) == 1 and b'g_src is NULL' in lib.slf_last_error()
        assert step(s, ref, None, a, c, a, a, None, a, a) == 1 and b'vz is NULL' in lib.slf_last_error()
        assert step(s, ref, None, a, c, a, a, a, None, a) == 1 and b'wall_temperature is NULL' in lib.slf_last_error()
        for omega in (0.0, 2.0, -1.0, float('nan')):
            bad = backend.thermal_params(omega, 0.5, [0.0] * 3, [True] * 3)
            assert step(s, ctypes.byref(bad), None, a, c, a, a, a, a, a) == 1 and b'omega_T' in lib.slf_last_error()
        assert lib.slf_thermal_init(s.module.handle, ref, None, None, a, a, a, c, s.stream.handle) == 1
        assert b'slf_thermal_init' in lib.slf_last_error() and b'T is NULL' in lib.slf_last_error()
        assert lib.slf_thermal_step(None, ref, None, a, c, a, a, a, a, a, s.stream.handle) == 1
        s.sync()
        backend.from_buf(addr, field)
        assert not field.any()                                           # and nothing was launched
        backend.free_buf(addr)
    finally:
        s.release()
    walled, periodic, map_fn = _accf.box_desc(grid, size, 'AB', 'single', 'guo', 'full', accel_field=True)
    s = BoxSim(backend, walled, periodic=periodic, node_map=map_fn(walled), accel_field=np.zeros((3,) + tuple(reversed(size))))
    try:
        a, c = P(s.gpu_rho), P(s.gpu_v[0])
        assert step(s, ref, None, a, c, a, a, a, a, a) == 1 and b'map is NULL' in lib.slf_last_error()
    finally:
        s.release()
    module = backend.build(make_box_desc(sym.D3Q15, size, precision='single', access_pattern='AB', visc=0.02,
                                         periodic_fused=[1, 1, 1]))            # a module only: nothing is launched on it
    addr = backend.alloc_buf(size=256)
    assert module.desc.lattice == hipabi.SLF_D3Q15
    p = P(addr)
    assert lib.slf_thermal_step(module.handle, ref, None, p, p, p, p, p, p, p, None) == 3          # SLF_ERR_UNSUPPORTED
    assert b'D3Q15' in lib.slf_last_error()
    backend.free_buf(addr)
