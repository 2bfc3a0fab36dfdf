"""The ternary Shan-Chen mixture (LBTernaryFluidShanChen, csrc/slf_sc3.hip) on the GPU through LBSimulationController and
the C ABI, against its numpy twin (tests/_scn_twin.py, held against the reference's sympy objects and -- with two components
-- against the CPU oracle bit for bit by tests/test_sc3_twin.py) and against itself across configurations.

Six distinct non-zero couplings, three distinct relaxation times and positive densities throughout (tests/_sc3.py).  With
the linear potential the kernels and the twin do the same IEEE operations in the same order: bits are demanded.  The
classic potential goes through expf on the device: the bound is the twin in float32 against the twin in float64 from the same
state, added up per step, times ORDER_FACTOR -- never anything the kernels return."""
import importlib

import numpy as np
import pytest

from sailfish_amd import hipabi
from tests import _sc, _sc3
from tests import _scn_twin as tw

pytestmark = pytest.mark.gpu

ORDER_FACTOR = 4      # what another evaluation of exp may cost over the twin's own rounding error (as tests/test_gpu_fe.py)
NAMES = ('rho', 'phi', 'theta')


def run(dim, size, steps, geo='LBGeometry', walls=False, forces=None, **kw):
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    sim_cls, _ = _sc3.make_sim(dim, walls=walls, forces=forces)
    extra = dict((k, kw.pop(k)) for k in ('subdomains', 'conn_axis') if k in kw)
    cfg = _sc3.config(dim, size, **kw)
    cfg.update(extra, max_iters=steps, quiet=True, perf_stats_every=0)
    ctrl = LBSimulationController(sim_cls, getattr(geo_mod, '%s%dD' % (geo, dim)), default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    return ctrl


def state(ctrl, dim):
    out = dict(('f%d' % k, _sc3.merged(ctrl, 'dist', k)) for k in range(3))
    for name in NAMES:
        out[name] = _sc3.merged(ctrl, name)
    for d in range(dim):
        out['v%d' % d] = _sc3.merged(ctrl, 'v%d' % d)
    return out


def twin_after(dim, size, steps, dtype, **kw):
    t = _sc3.make_twin(dim, size, dtype, **kw)
    for _ in range(steps):
        t.step()
    return t


def populations(t, s, pattern, steps):
    """[(twin's, device's)] populations per lattice the way the arrays hold them after `steps` steps: streamed -- or, after an
    odd number of in-place steps, the post-collision values of the last step in the node's own opposite slots."""
    if pattern == 'AA' and (steps & 1):
        opp = tw.opposite(t.grid)
        return [(t.post[k], s['f%d' % k][opp]) for k in range(3)]
    return [(t.f[k], s['f%d' % k]) for k in range(3)]


def assert_identical(t, s, dim, pattern, steps, what=''):
    """Populations of wet nodes, the three densities and v (the fields of the last step's pass in front), bit for bit."""
    wet = t.wet
    for k, (want, got) in enumerate(populations(t, s, pattern, steps)):
        assert got.dtype == want.dtype
        assert np.array_equal(got[:, wet], want[:, wet]), (what, 'lattice %d' % k)
    for k, name in enumerate(NAMES):
        assert np.array_equal(s[name][wet], t.field[k][wet]), (what, name)
    for d in range(dim):
        assert np.array_equal(s['v%d' % d][wet], t.v[d][wet]), (what, 'v%d' % d)


# ---- against the twin -------------------------------------------------------------------------------------------------------

# one wave plus two nodes in 2-D and 3-D; 130: the wave-edge words of row_push
SHAPES = [(2, (66, 5)), (3, (66, 4, 3)), (3, (130, 4, 3))]
SHAPE_IDS = ['D2Q9-66x5', 'D3Q19-66x4x3', 'D3Q19-130x4x3']


@pytest.mark.parametrize('steps', [20, 21])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('dim,size', SHAPES, ids=SHAPE_IDS)
def test_linear_potential_equals_the_twin_bit_for_bit(dim, size, precision, pattern, steps):
    ctrl = run(dim, size, steps, precision=precision, pattern=pattern)
    t = twin_after(dim, size, steps, _sc3.DTYPE[precision])
    assert_identical(t, state(ctrl, dim), dim, pattern, steps)


EXTRA = {
    'two couplings zero': dict(G13=0.0, G22=0.0),
    'body forces on lattices 0 and 2': dict(forces={0: [1e-4, -2e-4, 3e-4], 2: [-3e-4, 1e-4, 2e-4]}),
    'edm': dict(force='edm', forces={1: [2e-4, 1e-4, -1e-4]}),
}


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('case', sorted(EXTRA))
@pytest.mark.parametrize('dim,size', SHAPES[:2], ids=SHAPE_IDS[:2])
def test_extra_cases_equal_the_twin_bit_for_bit(dim, size, case, pattern):
    kw = dict(EXTRA[case])
    if 'forces' in kw:
        kw['forces'] = dict((k, a[:dim]) for k, a in kw['forces'].items())
    steps = 20
    ctrl = run(dim, size, steps, precision='single', pattern=pattern, **kw)
    t = twin_after(dim, size, steps, np.float32, **kw)
    assert_identical(t, state(ctrl, dim), dim, pattern, steps, case)
    if case == 'two couplings zero':
        assert list(ctrl.runners[0]._desc.sc3_G).count(0.0) == 3          # G13 = G31 and G22


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('dim,size', [(2, (40, 12)), (3, (40, 12, 6))], ids=['D2Q9', 'D3Q19'])
def test_walls_equal_the_twin_bit_for_bit(dim, size, precision, pattern):
    """Slabs on both y faces plus a block in the channel (as tests/_sc.make_wall_sim): the node-map path of every kernel."""
    for steps in (20, 21):
        ctrl = run(dim, size, steps, walls=True, precision=precision, pattern=pattern)
        assert not ctrl.runners[0]._desc.fluid_only
        t = twin_after(dim, size, steps, _sc3.DTYPE[precision], walls=True)
        assert t.wall.any() and t.wet.any()
        assert_identical(t, state(ctrl, dim), dim, pattern, steps, '%d steps' % steps)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('dim,size', SHAPES[:2], ids=SHAPE_IDS[:2])
def test_classic_potential_single_precision_within_the_twins_own_error(dim, size, pattern):
    """expf on the device, the C library's exp in the twin: per step the twin in float32 against the twin in float64 from the
    same state, added up over the steps, times ORDER_FACTOR."""
    steps = 20
    kw = dict(potential='classic', G11=-1.9, G33=-2.3)
    ctrl = run(dim, size, steps, precision='single', pattern=pattern, **kw)
    t = _sc3.make_twin(dim, size, np.float32, **kw)
    bound = dict(f=0.0, field=0.0, v=0.0)
    for _ in range(steps):
        w = t.astype(np.float64)
        t.step()
        w.step()
        bound['f'] += ORDER_FACTOR * max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(t.f, w.f))
        bound['field'] += ORDER_FACTOR * max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(t.field, w.field))
        bound['v'] += ORDER_FACTOR * max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(t.v, w.v))
    s = state(ctrl, dim)
    got = dict(f=max(float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) for a, b in populations(t, s, pattern, steps)),
               field=max(float(np.max(np.abs(s[n].astype(np.float64) - t.field[k].astype(np.float64)))) for k, n in enumerate(NAMES)),
               v=max(float(np.max(np.abs(s['v%d' % d].astype(np.float64) - t.v[d].astype(np.float64)))) for d in range(dim)))
    print(' '.join('%s %.2e (bound %.2e)' % (k, got[k], bound[k]) for k in sorted(got)))
    for k in got:
        assert got[k] <= bound[k], (k, got[k], bound[k])


# ---- against itself ----------------------------------------------------------------------------------------------------------

def _equal(a, b, wet, what):
    for k in sorted(a):
        x, y = a[k], b[k]
        if k[0] == 'f':
            assert np.array_equal(x[:, wet], y[:, wet]), (what, k)
        else:
            assert np.array_equal(x[wet], y[wet]), (what, k)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('dim,size', [(2, (66, 5)), (3, (66, 4, 3)), (2, (40, 12)), (3, (40, 12, 6))],
                         ids=['D2Q9', 'D3Q19', 'D2Q9-walls', 'D3Q19-walls'])
def test_fused_sweep_equals_the_three_kernels(dim, size, pattern, monkeypatch):
    """SLF_SC_FUSED=0 (the reference's three kernels) against the default: every slot of every array."""
    walls = size[1] == 12
    for steps in (20, 21):
        monkeypatch.delenv('SLF_SC_FUSED', raising=False)
        ctrl = run(dim, size, steps, walls=walls, precision='single', pattern=pattern)
        names = [k.name for k in ctrl.runners[0]._kernels_none[0][1]]
        a = state(ctrl, dim)
        monkeypatch.setenv('SLF_SC_FUSED', '0')
        ctrl = run(dim, size, steps, walls=walls, precision='single', pattern=pattern)
        three = [k.name for k in ctrl.runners[0]._kernels_none[0][1]]
        b = state(ctrl, dim)
        assert three == ['ShanChenCollideAndPropagate%d' % k for k in range(3)]
        assert names == ['ShanChenCollideAndPropagateFused']
        for k in sorted(a):
            assert np.array_equal(a[k], b[k]), (k, steps)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('dim,size', [(2, (66, 5)), (3, (66, 4, 3))], ids=['D2Q9', 'D3Q19'])
def test_ghost_layer_periodicity_equals_the_in_sweep_wrap(dim, size, precision, pattern):
    wet = np.ones(tuple(reversed(size)), dtype=bool)
    for steps in (20, 21):
        a = state(run(dim, size, steps, precision=precision, pattern=pattern), dim)
        b = state(run(dim, size, steps, precision=precision, pattern=pattern, fused=False), dim)
        _equal(a, b, wet, 'ghost-layer PBC, %d steps' % steps)


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('fused', [True, False], ids=['in-sweep wrap', 'ghost-layer kernels'])
def test_two_subdomains_equal_one(pattern, fused):
    """Two subdomains along y, z and x (two slabs of one process; x through ghost columns and index lists: the x-face
    planes of the binary kernels are not used) at 40 x 9 x 8, 20 steps."""
    dim, size, steps = 3, (40, 9, 8), 20
    wet = np.ones(tuple(reversed(size)), dtype=bool)
    kw = dict(precision='single', pattern=pattern, fused=fused)
    one = state(run(dim, size, steps, **kw), dim)
    for axis in 'yzx':
        ctrl = run(dim, size, steps, geo='EqualSubdomainsGeometry', subdomains=2, conn_axis=axis, **kw)
        assert len(ctrl.runners) == 2 and all(r._macro_links and r._links and r._nnx is None for r in ctrl.runners)
        _equal(one, state(ctrl, dim), wet, 'two subdomains along ' + axis)


# ---- the example -------------------------------------------------------------------------------------------------------------

def test_drop_example_runs_and_conserves_each_component():
    """examples/ternary_fluid/sc_drop_2d.py at 64 x 64 for 50 steps: finite fields; each component's total (the densities of
    the last step's pass in front: the rounding of the initial equilibria and of 49 collisions) moves by no more than
    ORDER_FACTOR times what the twin's own total moves by, run in float32 from the same state.  The twin and the kernels do
    the same operations but for exp (the C library's in the twin, expf on the device), which enters the forces only: the
    factor is what that and another order of the 4096-term sums may cost."""
    from sailfish_amd import geo as geo_mod, sym
    from sailfish_amd.controller import LBSimulationController
    mod = importlib.import_module('examples.ternary_fluid.sc_drop_2d')
    defaults = {}
    mod.SCSim.update_defaults(defaults)
    assert (defaults['lat_nx'], defaults['lat_ny'], defaults['G11'], defaults['G33'], defaults['sc_potential']) == \
        (256, 256, -4.8, -4.8, 'classic')
    size, steps = (64, 64), 50
    cfg = dict(lat_nx=size[0], lat_ny=size[1], max_iters=steps, quiet=True, perf_stats_every=0)
    ctrl = LBSimulationController(mod.SCSim, geo_mod.LBGeometry2D, default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    sim = ctrl.runners[0]._sim
    assert sim.rho.dtype == np.float32
    # the same initial state through the example's own subdomain class
    init = type('Init', (object,), {})()
    for name in NAMES:
        setattr(init, name, np.zeros((64, 64), dtype=np.float32))
    sub = type('S', (object,), dict(gx=64, gy=64))()
    hy, hx = np.mgrid[0:64, 0:64]
    mod.DropSubdomain.initial_conditions(sub, init, hx, hy)
    t = tw.ScTwin(sym.D2Q9, (64, 64), np.float32, [sym.relaxation_time(defaults['visc']), 1.0, 1.0],
                  [[-4.8, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, -4.8]], potential='classic')
    t.set_fields([getattr(init, n) for n in NAMES], [np.zeros((64, 64))] * 2)
    for _ in range(steps):
        t.step()
    for k, name in enumerate(NAMES):
        got = getattr(sim, name)
        assert np.all(np.isfinite(got))
        start = float(getattr(init, name).astype(np.float64).sum())
        drift = abs(float(got.astype(np.float64).sum()) - start)
        twin = abs(float(t.field[k].astype(np.float64).sum()) - start)
        bound = ORDER_FACTOR * twin
        print('%s: drift %.3e, twin %.3e, bound %.3e' % (name, drift, twin, bound))
        assert twin > 0.0 and drift <= bound
    assert all(np.all(np.isfinite(c)) for c in sim.v)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def _backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


BASE = dict(lattice=hipabi.SLF_D2Q9, model=hipabi.SLF_BGK, precision=4, access_pattern=hipabi.SLF_AB, lat_nx=18, lat_ny=10,
            arr_nx=32, arr_ny=10, tau=1.0, visc=1.0 / 6.0, tau_phi=0.9, fluid_only=0, nt_type_mask=3, nt_misc_shift=2,
            type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_FULL_BB])
TERNARY = dict(BASE, simtype=hipabi.SLF_SIM_SHAN_CHEN_TERNARY, tau_theta=1.1, sc3_G=[0.1, 0.2, 0.3, 0.2, 0.4, 0.5, 0.3, 0.5, 0.6])


def test_kernel_names_and_argument_lists_are_checked_per_simtype():
    from sailfish_amd.backend_hip import HIPFatalError
    backend = _backend()
    ternary = backend.build(hipabi.make_desc(**TERNARY))
    dim = 2
    # the ternary lists are accepted (addresses are only bound here, nothing is launched)
    backend.get_kernel(ternary, 'ShanChenPrepareMacroFields', None, [8] * (7 + dim) + [0], 'P' * (7 + dim) + 'i')
    for k in range(3):
        backend.get_kernel(ternary, 'ShanChenCollideAndPropagate%d' % k, None, [8] * (6 + dim) + [0], 'P' * (6 + dim) + 'i')
    backend.get_kernel(ternary, 'ShanChenCollideAndPropagateFused', None, [8] * (10 + dim) + [0], 'P' * (10 + dim) + 'i')
    backend.get_kernel(ternary, 'SetInitialConditions', None, [8] * (7 + dim), 'P' * (7 + dim))
    # single-fluid and binary-only names, and the binary argument lists, are refused naming the simtype
    for name in ('CollideAndPropagate', 'ComputeMacroFields', 'PrepareMacroFields', 'ShanChenCollideAndPropagateFusedV',
                 'ShanChenPrepareDensities', 'FreeEnergyPrepareMacroFields'):
        with pytest.raises(HIPFatalError, match='SLF_SIM_SHAN_CHEN_TERNARY'):
            backend.get_kernel(ternary, name, None, [8] * 6 + [0], 'PPPPPPi')
    for name, n in (('ShanChenPrepareMacroFields', 5 + dim), ('ShanChenCollideAndPropagate0', 5 + dim),
                    ('ShanChenCollideAndPropagate1', 5 + dim), ('ShanChenCollideAndPropagateFused', 7 + dim)):
        with pytest.raises(HIPFatalError, match='SLF_SIM_SHAN_CHEN_TERNARY.*ternary argument lists'):
            backend.get_kernel(ternary, name, None, [8] * n + [0], 'P' * n + 'i')
    with pytest.raises(HIPFatalError, match='SLF_SIM_SHAN_CHEN_TERNARY.*ternary argument lists'):
        backend.get_kernel(ternary, 'SetInitialConditions', None, [8] * (5 + dim), 'P' * (5 + dim))
    # the other way round
    binary = backend.build(hipabi.make_desc(**dict(BASE, simtype=hipabi.SLF_SIM_SHAN_CHEN_BINARY, sc_G=[0.0, 1.0, 1.0, 0.0])))
    single = backend.build(hipabi.make_desc(**dict(BASE, simtype=hipabi.SLF_SIM_LBM)))
    for module in (binary, single):
        with pytest.raises(HIPFatalError, match='ShanChenCollideAndPropagate2.*SLF_SIM_SHAN_CHEN_TERNARY'):
            backend.get_kernel(module, 'ShanChenCollideAndPropagate2', None, [8] * (6 + dim) + [0], 'P' * (6 + dim) + 'i')
    with pytest.raises(HIPFatalError, match='signature'):
        backend.get_kernel(binary, 'ShanChenCollideAndPropagate0', None, [8] * (6 + dim) + [0], 'P' * (6 + dim) + 'i')


def test_body_force_of_lattice_two_is_set_through_the_abi():
    from sailfish_amd.backend_hip import HIPFatalError
    backend = _backend()
    ternary = backend.build(hipabi.make_desc(**TERNARY))
    backend.set_body_force(ternary, [1e-5, 0.0, 0.0], 2)
    backend.set_body_force(ternary, [1e-5, 0.0, 0.0], 1)
    binary = backend.build(hipabi.make_desc(**dict(BASE, simtype=hipabi.SLF_SIM_SHAN_CHEN_BINARY, sc_G=[0.0, 1.0, 1.0, 0.0])))
    with pytest.raises(HIPFatalError, match='lattice 2'):
        backend.set_body_force(binary, [1e-5, 0.0, 0.0], 2)


MODULE_REFUSALS = [
    (dict(model=hipabi.SLF_MRT), 'ternary Shan-Chen: --model=mrt'),
    (dict(node_addressing=hipabi.SLF_ADDR_INDIRECT, dist_stride=4096), 'node_addressing=indirect'),
    (dict(type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_HALF_BB]), 'NTFullBBWall'),
    (dict(type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_EQUILIBRIUM_DENSITY]), 'NTFullBBWall'),
    (dict(incompressible=hipabi.SLF_DENSITY_ROUNDOFF), 'minimize_roundoff'),
    (dict(tau_theta=0.5), 'tau_theta'),
]


@pytest.mark.parametrize('over,message', MODULE_REFUSALS, ids=[m for _, m in MODULE_REFUSALS])
def test_refused_at_module_creation(over, message):
    from sailfish_amd.backend_hip import HIPFatalError
    backend = _backend()
    with pytest.raises(HIPFatalError, match=message):
        backend.build(hipabi.make_desc(**dict(TERNARY, **over)))


def test_x_face_planes_are_refused_by_name():
    from sailfish_amd.backend_hip import HIPFatalError
    backend = _backend()
    kw = dict(TERNARY, lattice=hipabi.SLF_D3Q19, lat_nz=6, arr_nz=6)
    module = backend.build(hipabi.make_desc(**kw))
    lib = hipabi.load()
    rc = lib.slf_module_set_xface_planes(module.handle, 0, 8, 8, 8, 8)
    assert rc != 0 and b'SLF_SIM_SHAN_CHEN_TERNARY' in lib.slf_last_error()
    assert HIPFatalError is not None
