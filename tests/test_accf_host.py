"""Body forces that depend on position, host layer: LBForcedSim turns DynamicValue expressions of S.gx / S.gy / S.gz into an
acceleration field, the descriptor carries accel_field, the runner evaluates the field at global coordinates, uploads it
once and hands it to the module, and everything no kernel serves is refused by name.  No GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import sailfish  # noqa: F401  (the sailfish.* aliases)
from sailfish_amd import geo as geo_mod
from sailfish_amd import hipabi
from sailfish_amd.lb_base import LBForcedSim, LBSim
from sailfish_amd.lb_single import LBFluidSim
from sailfish_amd.node_type import DynamicValue, NTWallTMS
from sailfish_amd.subdomain import Subdomain2D, Subdomain3D, SubdomainSpec2D
from sailfish_amd.sym import S
from tests import _host

HAVE_REF = os.path.isdir('/root/reference/examples')


def full_cfg(sim_cls, geo, cfg):
    """Every option at its declared default (the example's own included), as the controller's parser delivers them."""
    from sailfish_amd.controller import LBSimulationController
    defaults = {}
    sim_cls.update_defaults(defaults)
    defaults.update(cfg)
    ctrl = LBSimulationController(sim_cls, geo, default_config=defaults)
    full = dict((k, v) for k, v in vars(ctrl._config_parser.parse([])).items() if not k.startswith('_'))
    full.update(defaults)
    return full


def runners_of(sim_cls, dim, geo, cfg):
    if isinstance(geo, str):
        geo = getattr(geo_mod, geo)
    _, specs, runners = _host.build_runners(sim_cls, dim, geo, full_cfg(sim_cls, geo, cfg))
    for r in runners:
        r._init_geometry()
        r._sim.init_fields(r)
        r._subdomain.init_fields(r._sim)
    return specs, runners


def quad_geometry(cx, cy):
    class Geo(geo_mod.LBGeometry2D):
        def subdomains(self, n=None):
            gx, gy = self.gsize
            return [SubdomainSpec2D((x0, y0), (x1 - x0, y1 - y0))
                    for y0, y1 in ((0, cy), (cy, gy)) for x0, x1 in ((0, cx), (cx, gx))]
    return Geo


def mill():
    from examples.four_rolls_mill import FourRollsMill
    return FourRollsMill


def mill_expressions(cfg, hx, hy):
    """The mill's acceleration from its own formula, numpy, float64."""
    kx, ky = 2.0 * np.pi * cfg['lambda_x'] / cfg['lat_nx'], 2.0 * np.pi * cfg['lambda_y'] / cfg['lat_ny']
    ksq = kx * kx + ky * ky
    amp = cfg['visc'] * ksq * cfg['max_v'] / np.sqrt(ksq)
    return [-amp * ky * np.sin(ky * hy) * np.cos(kx * hx), amp * kx * np.sin(kx * hx) * np.cos(ky * hy)]


MILL_CFG = dict(lat_nx=40, lat_ny=24, visc=0.05, max_v=0.02, lambda_x=1, lambda_y=2)


def real_and_rest(r, field):
    """(values at the real nodes [dim, ny, nx], everything else flattened)"""
    sp = r._spec
    box = tuple(slice(0, n) for n in r._lat_size)
    real = np.zeros(field.shape[1:], dtype=bool)
    real[box][sp._nonghost_slice] = True
    shape = tuple(reversed(sp.size))
    return np.stack([c[real].reshape(shape) for c in field]), np.stack([c[~real] for c in field])


# ---- LBForcedSim ------------------------------------------------------------------------------------------------------------

def test_position_dependent_force_is_accepted_and_described():
    specs, (r,) = runners_of(mill(), 2, 'LBGeometry2D', MILL_CFG)
    sim = r._sim
    assert sim.has_accel_field and r.config.space_dependence and not sim.time_dependent_force
    assert sim.body_force_at(0) is None                   # no uniform part
    d = r._module_desc()
    assert d.accel_field == 1 and d.has_force == 1 and list(d.accel) == [0.0, 0.0, 0.0]
    assert d.struct_size == hipabi.ctypes.sizeof(hipabi.SlfModuleDesc)
    plain = hipabi.make_desc()
    assert plain.accel_field == 0


@pytest.mark.parametrize('precision', ['single', 'double'])
def test_runner_field_is_the_expression_at_global_coordinates(precision):
    cfg = dict(MILL_CFG, precision=precision)
    _, (one,) = runners_of(mill(), 2, 'LBGeometry2D', cfg)
    whole, rest = real_and_rest(one, one.accel_field_host())
    dtype = np.float32 if precision == 'single' else np.float64
    assert whole.dtype == dtype and whole.shape == (2, 24, 40)
    hy, hx = np.mgrid[0:24, 0:40].astype(np.float64)
    want = mill_expressions(cfg, hx, hy)
    for k in range(2):
        # evaluated in float64 (sympy's numpy code against numpy: a few ulps of float64; where a sine crosses zero the two
        # differ by the rounding of its argument, 1e-16 of an amplitude of 1e-4), rounded once
        assert np.allclose(whole[k].astype(np.float64), want[k], rtol=2e-7 if precision == 'single' else 1e-12, atol=1e-17)
        assert np.ptp(whole[k]) > 0
    assert rest.size > 0 and np.all(rest == 0)            # ghost layer and padding
    # 2 x 2 subdomains: every runner holds its window of the undivided field, bit for bit
    specs, four = runners_of(mill(), 2, quad_geometry(17, 10), cfg)
    assert len(four) == 4
    for r in four:
        part, rest = real_and_rest(r, r.accel_field_host())
        x0, y0 = r._spec.location
        nx, ny = r._spec.size
        assert np.array_equal(part, whole[:, y0:y0 + ny, x0:x0 + nx])
        assert np.all(rest == 0)


class Box3(Subdomain3D):
    tms = False

    def boundary_conditions(self, hx, hy, hz):
        if self.tms:
            self.set_node((hy == 0) | (hy == self.gy - 1), NTWallTMS)

    def initial_conditions(self, sim, hx, hy, hz):
        sim.rho[:] = 1.0


class TmsBox3(Box3):
    tms = True


def forced3(forces, subdomain=Box3):
    class Sim3(LBFluidSim, LBForcedSim):
        def __init__(self, config):
            super(Sim3, self).__init__(config)
            for f in forces:
                self.add_body_force(f)
    Sim3.subdomain = subdomain
    return Sim3


CFG3 = dict(lat_nx=10, lat_ny=6, lat_nz=5, periodic_x=True, periodic_y=True, periodic_z=True, precision='double', visc=0.05)
FIELD3 = DynamicValue(1e-5 * S.gx, 2e-5 * S.gy * S.gx, 3e-5 * S.gz + 1e-6)


def test_several_forces_add_up():
    from sympy import sin
    forces = [FIELD3, (1e-6, 0.0, -2e-6), DynamicValue(0.0, 4e-6 * S.gz, 0.0), DynamicValue(1e-6 * sin(S.time), 0.0, 0.0),
              (0.0, 5e-7, 0.0)]
    _, (r,) = runners_of(forced3(forces), 3, 'LBGeometry3D', dict(CFG3, dt_per_lattice_time_unit=0.5))
    sim = r._sim
    assert sim.has_accel_field and sim.time_dependent_force
    d = r._module_desc()
    assert d.accel_field == 1 and d.has_force == 1
    assert list(d.accel) == [1e-6, 5e-7, -2e-6]                          # uniform and time-only parts, at iteration 0
    assert np.allclose(sim.body_force_at(2), [1e-6 + 1e-6 * np.sin(1.0), 5e-7, -2e-6], rtol=1e-14)
    z, y, x = [c.astype(np.float64) for c in np.mgrid[0:5, 0:6, 0:10]]
    at = sim.accel_field_at((x.ravel(), y.ravel(), z.ravel()))
    assert at.shape == (3, 300) and at.dtype == np.float64
    want = [1e-5 * x, 2e-5 * y * x + 4e-6 * z, 3e-5 * z + 1e-6]
    real, _ = real_and_rest(r, r.accel_field_host())
    for k in range(3):
        assert np.allclose(at[k], want[k].ravel(), rtol=1e-14, atol=1e-22)
        assert np.array_equal(real[k], at[k].reshape(5, 6, 10))           # double precision: no rounding on the way


def test_refused_forms_of_add_body_force():
    from sympy import sin
    bare = forced3([])(_host.make_config(3, **CFG3))
    with pytest.raises(NotImplementedError, match='need a backend that reads an acceleration field'):
        bare.add_body_force(FIELD3)                      # a configuration no backend with the field has put its option into
    assert not bare.has_accel_field
    cfg = _host.make_config(3, hip_accel_field=True, **CFG3)
    sim = forced3([])(cfg)
    with pytest.raises(NotImplementedError, match='both position and time'):
        sim.add_body_force(DynamicValue(1e-5 * S.gx * sin(S.time), 0.0, 0.0))
    with pytest.raises(NotImplementedError, match='accel=True'):
        sim.add_body_force(FIELD3, accel=False)
    with pytest.raises(NotImplementedError, match='grid=0'):
        sim.add_body_force(FIELD3, grid=1)
    with pytest.raises(NotImplementedError, match='time-dependent body forces'):
        sim.add_body_force(DynamicValue(sin(S.time), 0.0, 0.0), grid=1)
    assert not sim.has_accel_field


# ---- refusals ----------------------------------------------------------------------------------------------------------------

REFUSALS = [
    (dict(lattice=hipabi.SLF_D3Q15), 'D3Q15'),
    (dict(lattice=hipabi.SLF_D3Q27), 'D3Q27'),
    (dict(model=hipabi.SLF_ELBM), '--model=elbm'),
    (dict(regularized=1), '--regularized'),
    (dict(subgrid=1), '--subgrid'),
    (dict(incompressible=hipabi.SLF_DENSITY_ROUNDOFF), '--minimize_roundoff'),
    (dict(type_kind=[0, 1, hipabi.SLF_NK_WALL_TMS]), 'NTWallTMS'),
    (dict(node_addressing=hipabi.SLF_ADDR_INDIRECT), '--node_addressing=indirect'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_BINARY), 'Shan-Chen'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_SINGLE), 'Shan-Chen'),
    (dict(simtype=hipabi.SLF_SIM_FREE_ENERGY), 'free-energy'),
    (dict(simtype=hipabi.SLF_SIM_SHAN_CHEN_TERNARY), 'ternary Shan-Chen'),
]


@pytest.mark.parametrize('extra,word', REFUSALS, ids=[w for _, w in REFUSALS])
def test_check_module_desc_refuses_by_name(extra, word):
    from sailfish_amd.lb_binary import LBBinaryFluidFreeEnergy, LBBinaryFluidShanChen
    from sailfish_amd.lb_single import LBSingleFluidShanChen
    from sailfish_amd.lb_ternary import LBTernaryFluidShanChen
    base = dict(lattice=hipabi.SLF_D3Q19, model=hipabi.SLF_BGK, type_kind=[0, 1, 4])
    classes = {hipabi.SLF_SIM_SHAN_CHEN_BINARY: LBBinaryFluidShanChen, hipabi.SLF_SIM_SHAN_CHEN_SINGLE: LBSingleFluidShanChen,
               hipabi.SLF_SIM_FREE_ENERGY: LBBinaryFluidFreeEnergy, hipabi.SLF_SIM_SHAN_CHEN_TERNARY: LBTernaryFluidShanChen}
    cls = classes.get(extra.get('simtype'), LBFluidSim)
    cls.check_module_desc(dict(base, **extra))                          # without a field: not this refusal's business
    with pytest.raises(NotImplementedError) as e:
        cls.check_module_desc(dict(base, accel_field=1, **extra))
    assert 'depend on position' in str(e.value) and word in str(e.value)
    LBSim.check_accel_field(dict(base, accel_field=1))                  # the served base case


@pytest.mark.parametrize('cfg,word', [
    (dict(grid='D3Q15'), 'D3Q15'), (dict(grid='D3Q27'), 'D3Q27'), (dict(model='elbm'), '--model=elbm'),
    (dict(regularized=True), '--regularized'), (dict(subgrid='les-smagorinsky'), '--subgrid'),
    (dict(minimize_roundoff=True), '--minimize_roundoff'), (dict(node_addressing='indirect'), '--node_addressing=indirect'),
    (dict(tms=True), 'NTWallTMS')], ids=lambda v: v if isinstance(v, str) else '')
def test_runner_refuses_before_anything_is_built(cfg, word):
    cfg = dict(cfg)
    sub = TmsBox3 if cfg.pop('tms', False) else Box3
    if sub is TmsBox3:
        cfg.update(periodic_y=False)
    _, (r,) = runners_of(forced3([FIELD3], sub), 3, 'LBGeometry3D', dict(CFG3, **cfg))
    with pytest.raises(NotImplementedError) as e:
        r._module_desc()
    assert 'depend on position' in str(e.value) and word in str(e.value)


def test_x_faces_of_a_field_module_go_through_ghost_columns():
    """The x-face buffers are read and written by the whole-row kernels, which a module with a field is routed around."""
    from sailfish_amd import sym, xface
    _, (r,) = runners_of(forced3([FIELD3]), 3, 'LBGeometry3D', dict(CFG3, precision='single'))
    d = r._module_desc()
    assert not xface.supported(sym.D3Q19, d)
    d.accel_field = 0
    assert xface.supported(sym.D3Q19, d)


# ---- the runner's call sequence ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_field_is_uploaded_once_before_the_first_launch_and_no_resident_path(pattern):
    from sailfish_amd.controller import LBSimulationController
    from tests import _accf_backend
    del _accf_backend.LOG[:]
    cfg = dict(MILL_CFG, access_pattern=pattern, precision='single', max_iters=20, quiet=True, perf_stats_every=0, gpus=[0],
               backends='tests._accf_backend', output='', err_every=1000)
    ctrl = LBSimulationController(mill(), geo_mod.EqualSubdomainsGeometry2D, default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    (r,) = ctrl.runners
    log = list(_accf_backend.LOG)
    kinds = [e[0] for e in log]
    assert log[0] == ('build', 1)
    assert kinds.count('set_accel_field') == 1
    first_run = kinds.index('run')
    assert kinds.index('set_accel_field') < first_run
    _, module, addr, field = log[kinds.index('set_accel_field')]
    assert module is r.module and addr == r._gpu_accel_field
    host = r.accel_field_host()
    assert np.array_equal(field.reshape(host.shape), host) and np.ptp(field) > 0
    names = [e[1] for e in log if e[0] in ('get_kernel', 'run')]
    assert 'CollideAndPropagateResident' not in names
    assert [e[1] for e in log if e[0] == 'run'].count('CollideAndPropagate') == 20      # one launch per step
    assert r._resident_setup() is None


# ---- the reference's own example ------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not HAVE_REF, reason='/root/reference not available on this machine')
def test_reference_four_rolls_mill_loads_unchanged():
    """The reference's examples/four_rolls_mill.py, imported unchanged against the `sailfish` alias package (it imports its
    sibling taylor_green_2d by bare name): options parse, the geometry builds, and the field the runner uploads equals the
    example's own expressions at every real node."""
    ref = '/root/reference/examples'
    sys.path.insert(0, ref)
    try:
        spec = importlib.util.spec_from_file_location('refexample_four_rolls_mill', os.path.join(ref, 'four_rolls_mill.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(ref)
        sys.modules.pop('taylor_green_2d', None)
    sim_cls = mod.FourRollsMill
    cfg = dict(lat_nx=48, lat_ny=32, precision='double')
    _, (r,) = runners_of(sim_cls, 2, 'LBGeometry2D', cfg)
    d = r._module_desc()
    assert d.accel_field == 1 and d.has_force == 1 and d.lattice == hipabi.SLF_D2Q9
    real, rest = real_and_rest(r, r.accel_field_host())
    c = r.config
    hy, hx = np.mgrid[0:32, 0:48].astype(np.float64)
    want = mill_expressions(dict(lat_nx=48, lat_ny=32, visc=c.visc, max_v=c.max_v, lambda_x=c.lambda_x, lambda_y=c.lambda_y),
                            hx, hy)
    for k in range(2):
        assert np.allclose(real[k], want[k], rtol=1e-12, atol=1e-17) and np.ptp(real[k]) > 0
    assert np.all(rest == 0)


def test_placement_probe_is_the_plain_sweep():
    """The placement probe times the plain fluid sweep on a module of its own, which never sees the field: built with
    accel_field it would refuse to launch."""
    from sailfish_amd import placement

    class Built(Exception):
        pass

    class Backend(object):
        def build(self, d):
            raise Built(d)

    _, (r,) = runners_of(forced3([FIELD3]), 3, 'LBGeometry3D', dict(CFG3, precision='single'))
    desc = r._module_desc()
    assert desc.accel_field == 1
    with pytest.raises(Built) as e:
        placement.probe_sweep(Backend(), desc, 3, 4096, 8192, 1 << 20, None)
    probe = e.value.args[0]
    assert probe.accel_field == 0 and probe.has_force == 0 and probe.lat_nx == desc.lat_nx
    assert desc.accel_field == 1                       # the runner's descriptor is untouched
