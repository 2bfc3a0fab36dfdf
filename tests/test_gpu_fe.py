"""The free-energy binary fluid (LBBinaryFluidFreeEnergy, csrc/slf_fe.hip) on the GPU, against its numpy twin
(tests/_fe_twin.py, itself held against the reference's sympy objects by tests/test_fe_twin.py) and against itself across
configurations.  Tolerances are sized from the twin -- the twin in the kernels' format against the twin in the next wider
one -- never from what the kernels return."""
import os

import numpy as np
import pytest

from sailfish_amd import hipabi
from tests import _fe
from tests import _fe_twin as tw

pytestmark = pytest.mark.gpu

ORDER_FACTOR = 4      # what another summation order may cost over the twin's own rounding error


def run(dim, size, steps, geo='LBGeometry', **kw):
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    sim_cls, _ = _fe.make_sim(dim, walls=kw.get('walls', False))
    extra = dict((k, kw.pop(k)) for k in ('subdomains', 'conn_axis', 'subdomains_y', 'subdomains_z') if k in kw)
    cfg = _fe.config(dim, size, **kw)
    cfg.update(extra, max_iters=steps, quiet=True, perf_stats_every=0)
    ctrl = LBSimulationController(sim_cls, getattr(geo_mod, '%s%dD' % (geo, dim)), default_config=cfg)
    ctrl.run(ignore_cmdline=True)
    return ctrl


def state(ctrl, dim):
    out = {'f': _fe.merged(ctrl, 'dist', 0), 'g': _fe.merged(ctrl, 'dist', 1)}
    for name in ('rho', 'phi', 'phi_laplacian'):
        out[name] = _fe.merged(ctrl, name)
    for d in range(dim):
        out['v%d' % d] = _fe.merged(ctrl, 'v%d' % d)
    return out


def _wider(dtype):
    if dtype is np.float32:
        return np.float64
    return np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else None


def _step_error(t):
    """One step of the twin `t` (advanced) against the same step in the next wider format from the same state: the largest
    difference per quantity."""
    wide = _wider(t.R)
    if wide is None:          # no wider format: a step is some 60 roundings per population, each half an ulp of values below 2
        t.step()
        return dict((k, 64 * float(np.finfo(t.R).eps)) for k in ('f', 'g', 'phi', 'lap', 'v'))
    w = t.astype(wide)
    t.step()
    w.step()
    wet = t.wet
    err = {'f': np.max(np.abs(t.f.astype(wide) - w.f)[:, wet]), 'g': np.max(np.abs(t.g.astype(wide) - w.g)[:, wet]),
           'phi': np.max(np.abs(t.phi.astype(wide) - w.phi)), 'lap': np.max(np.abs(t.lap.astype(wide) - w.lap)[wet]),
           'v': max(np.max(np.abs(a.astype(wide) - b)[wet]) for a, b in zip(t.v, w.v))}
    return dict((k, float(v)) for k, v in err.items())


def _compare(ctrl, t, dim, bound, fields_of_step_before=True):
    """Populations of the wet nodes after the run; phi everywhere (walls: the wetting value), v and the Laplacian of the wet
    nodes -- the fields are those of the last step, i.e. of the twin one step back (`tb`)."""
    s = state(ctrl, dim)
    wet = t.wet
    got = {'f': np.max(np.abs(s['f'].astype(np.float64) - t.f.astype(np.float64))[:, wet]),
           'g': np.max(np.abs(s['g'].astype(np.float64) - t.g.astype(np.float64))[:, wet]),
           'phi': np.max(np.abs(s['phi'].astype(np.float64) - t.phi.astype(np.float64))),
           'lap': np.max(np.abs(s['phi_laplacian'].astype(np.float64) - t.lap.astype(np.float64))[wet]),
           'v': max(np.max(np.abs(s['v%d' % d].astype(np.float64) - t.v[d].astype(np.float64))[wet]) for d in range(dim))}
    print(' '.join('%s %.2e (bound %.2e)' % (k, got[k], bound[k]) for k in sorted(got)))
    for k in got:
        assert got[k] <= bound[k], (k, got[k], bound[k])
    return s


def _run_twin(dim, size, steps, dtype, **kw):
    """The twin after `steps` steps and the accumulated bound: ORDER_FACTOR times the sum of its per-step errors."""
    t = _fe.make_twin(dim, size, dtype, **kw)
    total = dict((k, 0.0) for k in ('f', 'g', 'phi', 'lap', 'v'))
    for _ in range(steps):
        e = _step_error(t)
        for k in total:
            total[k] += ORDER_FACTOR * e[k]
    return t, total


# ---- one collision ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('dim,size', [(2, (66, 5)), (3, (66, 4, 3))], ids=['D2Q9', 'D3Q19'])
def test_one_collision_against_the_twin(golden_dir, dim, size, precision):
    """A periodic box every node of which carries the same populations is invariant under streaming: one step leaves every
    node with the post-collision state.  The fixture's states with zero gradient (a uniform phi has none), populations
    off equilibrium; a 66-node row is one wave plus two nodes.  Bound: the twin in the kernels' precision against the twin
    in the next wider format, times ORDER_FACTOR."""
    grid, dtype = _fe.GRID[dim], _fe.DTYPE[precision]
    G = np.load(os.path.join(golden_dir, 'arith_fe_%s.npz' % grid.__name__))
    P = dict((k, float(G[k])) for k in ('A', 'kappa', 'Gamma', 'tau_a', 'tau_b'))
    P['tau_phi'] = 0.9
    ctrl = run(dim, size, 1, precision=precision, **P)
    r = ctrl.runners[0]
    b = r.backend
    sel = np.nonzero(np.all(G['grad'] == 0, axis=1))[0]
    assert len(sel) >= 20 and (G['phi'][sel] < -1).any() and (G['phi'][sel] > 1).any()
    rng = np.random.RandomState(11)
    wide = _wider(dtype)
    worst = dict(f=0.0, g=0.0)
    tol = dict(f=0.0, g=0.0)
    shape = [grid.Q] + list(r._physical_size)
    nodes = int(np.prod(r._physical_size))
    for k in sel:
        v = [G['v'][k, d] for d in range(dim)]
        zero = [0.0] * dim
        # off equilibrium by a few percent, moments unchanged to rounding in the formats' own terms
        f0 = tw.feq_fluid(grid, G['rho'][k], G['phi'][k], 0.0, v, zero, P['A'], P['kappa'], np.float64) * (1 + 0.03 * rng.uniform(-1, 1, grid.Q))
        g0 = tw.feq_order(grid, G['phi'][k], 0.0, v, P['A'], P['kappa'], P['Gamma'], np.float64) + 0.01 * rng.uniform(-1, 1, grid.Q)
        f0, g0 = f0.astype(dtype), g0.astype(dtype)
        phi = tw.density(g0[:, None])
        lap, grad = tw.stencil(grid, lambda i: phi, phi, dtype)       # of a uniform field: zero up to the rounding of its sums
        want = tw.collide(grid, f0[:, None], g0[:, None], phi, lap, grad, dtype, **P)
        if wide is not None:
            pw = phi.astype(wide)
            lw, gw = tw.stencil(grid, lambda i: pw, pw, wide)
            ref = tw.collide(grid, f0[:, None].astype(wide), g0[:, None].astype(wide), pw, lw, gw, wide, **P)
            for name in ('f', 'g'):
                tol[name] = max(tol[name], ORDER_FACTOR * float(np.max(np.abs(want[name].astype(wide) - ref[name]))))
        else:
            tol = dict(f=ORDER_FACTOR * 16 * np.finfo(dtype).eps, g=ORDER_FACTOR * 16 * np.finfo(dtype).eps)
        for lattice, pops in ((0, f0), (1, g0)):
            full = np.zeros((grid.Q, r._dist_stride), dtype=dtype)
            full[:, :nodes] = pops[:, None]
            b.to_buf(r.gpu_dist(lattice, 0), full)
        b.set_iteration(0)
        macro, sweeps = r._kernels_full[0]
        for kern in [macro] + list(sweeps):
            b.run_kernel(kern, None, r._calc_stream)
        b.sync_stream(r._calc_stream)
        for lattice, name in ((0, 'f'), (1, 'g')):
            raw = np.zeros((grid.Q, r._dist_stride), dtype=dtype)
            b.from_buf(r.gpu_dist(lattice, 1), raw)
            out = raw[:, :nodes].reshape(shape)[(slice(None),) + tuple(r._spec._nonghost_slice)].reshape(grid.Q, -1)
            assert np.all(out == out[:, :1])                   # every node did the same arithmetic
            worst[name] = max(worst[name], float(np.max(np.abs(out[:, 0].astype(np.float64) - want[name][:, 0].astype(np.float64)))))
    print('%s %s: |f - twin| %.3e (tol %.3e), |g - twin| %.3e (tol %.3e)' % (grid.__name__, precision, worst['f'], tol['f'],
                                                                             worst['g'], tol['g']))
    assert worst['f'] <= tol['f'] and worst['g'] <= tol['g']


# ---- whole steps ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dim,size', [(2, (66, 10)), (3, (66, 6, 5))], ids=['D2Q9', 'D3Q19'])
def test_twenty_steps_against_the_twin(dim, size):
    """Double precision, AB, a random smooth phi in [-1, 1]: every population of both lattices, phi, v and the Laplacian
    within ORDER_FACTOR times the twin's own per-step rounding error (float64 against longdouble), added up over the
    steps.  The fields are those of the last step: the twin's after 19 steps."""
    steps = 20
    ctrl = run(dim, size, steps)
    t, bound = _twin_fields_of_last_step(dim, size, steps, np.float64)
    _compare(ctrl, t, dim, bound)


# ---- walls and wetting ------------------------------------------------------------------------------------------------------

WALL_BOXES = [(3, (20, 12, 10)), (2, (34, 12))]


def _twin_fields_of_last_step(dim, size, steps, dtype, **kw):
    """The twin after `steps` steps with the fields its last step stored (phi, v, Laplacian before that step's collision),
    and the accumulated bound."""
    t, bound = _run_twin(dim, size, steps, dtype, **kw)
    tb, _ = _run_twin(dim, size, steps - 1, dtype, **kw)
    tb.macro()
    lap, grad = tb._stencil(tb.phi)
    r = tw.collide(tb.grid, tb.f, tb.g, tb.phi, lap, grad, tb.R, **tb.c)
    t.phi, t.lap, t.v = tb.phi, np.where(tb.wet, lap, tb.lap), [np.where(tb.wet, a, b) for a, b in zip(r['v'], tb.v)]
    return t, bound


@pytest.mark.parametrize('phase', [0.0, 0.1])
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('dim,size', WALL_BOXES, ids=['D3Q19', 'D2Q9'])
def test_wetting_walls_against_the_twin(dim, size, order, phase):
    """Full-way walls on both faces of the last axis, 10 steps, double precision.  phi of a wall node is a value copy: phi
    of its helper node minus the constant -- checked exactly against the device's own phi."""
    steps = 10
    ctrl = run(dim, size, steps, walls=True, order=order, phase=phase)
    t, bound = _twin_fields_of_last_step(dim, size, steps, np.float64, walls=True, order=order, phase=phase)
    s = _compare(ctrl, t, dim, bound)
    phi = s['phi']
    shift = np.float64(float(order) * float(phase))
    assert np.array_equal(phi[0], phi[order] - shift) and np.array_equal(phi[-1], phi[-1 - order] - shift)
    assert phase == 0.0 or not np.array_equal(phi[0], phi[order])


# ---- bit for bit between configurations ---------------------------------------------------------------------------------

def _equal(a, b, wet, what):
    for k in sorted(a):
        x, y = a[k], b[k]
        if k in ('f', 'g'):
            assert np.array_equal(x[:, wet], y[:, wet]), (what, k)
        elif k == 'phi':
            assert np.array_equal(x, y), (what, k)
        else:
            assert np.array_equal(x[wet], y[wet]), (what, k)


def _wet(dim, size):
    wet = np.ones(tuple(reversed(size)), dtype=bool)
    wet[0] = wet[-1] = False
    return wet


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('dim,size', WALL_BOXES, ids=['D3Q19', 'D2Q9'])
def test_in_place_equals_two_copy(dim, size, precision):
    """AB == AA after 10 steps (populations and the fields of the last step) and after 11 (the fields of the last step: the
    in-place arrays then hold the populations un-streamed)."""
    wet = _wet(dim, size)
    for steps in (10, 11):
        a = state(run(dim, size, steps, walls=True, phase=0.1, precision=precision, pattern='AB'), dim)
        b = state(run(dim, size, steps, walls=True, phase=0.1, precision=precision, pattern='AA'), dim)
        if steps & 1:
            del a['f'], a['g'], b['f'], b['g']
        _equal(a, b, wet, 'AA after %d steps' % steps)


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('dim,size', WALL_BOXES, ids=['D3Q19', 'D2Q9'])
def test_ghost_layer_periodicity_and_subdomains_equal_one_subdomain(dim, size, pattern, precision):
    """In-sweep wrap == ghost-layer PBC kernels; one subdomain == two along x, y, z == 2 x 2 along (y, z): same-process
    groups (controller.LocalGroup), phi through the macro exchange, at start-up too."""
    wet = _wet(dim, size)
    kw = dict(walls=True, phase=0.1, precision=precision, pattern=pattern)
    steps = 10
    one = state(run(dim, size, steps, **kw), dim)
    _equal(one, state(run(dim, size, steps, fused=False, **kw), dim), wet, 'ghost-layer PBC')
    for axis in 'xyz'[:dim]:
        ctrl = run(dim, size, steps, geo='EqualSubdomainsGeometry', subdomains=2, conn_axis=axis, **kw)
        assert len(ctrl.runners) == 2 and all(r._macro_links for r in ctrl.runners)
        _equal(one, state(ctrl, dim), wet, 'two subdomains along ' + axis)
        _equal(one, state(run(dim, size, steps, geo='EqualSubdomainsGeometry', subdomains=2, conn_axis=axis, fused=False, **kw),
                          dim), wet, 'two subdomains along %s, ghost-layer PBC' % axis)
    if dim == 3:
        from sailfish_amd.controller import LBSimulationController
        from tests.test_halo_oracle import _block_geometry
        sim_cls, _ = _fe.make_sim(dim, walls=True)
        cfg = _fe.config(dim, size, **kw)
        cfg.update(max_iters=steps, quiet=True, perf_stats_every=0)
        ctrl = LBSimulationController(sim_cls, _block_geometry(3, [[], [5], [5]]), default_config=cfg)
        ctrl.run(ignore_cmdline=True)
        assert len(ctrl.runners) == 4
        _equal(one, state(ctrl, dim), wet, '2 x 2 subdomains along (y, z)')


# ---- conservation -----------------------------------------------------------------------------------------------------------

def test_mass_and_order_parameter_are_conserved():
    """Periodic D3Q19 32 x 8 x 8, single precision, 200 steps.  A collision changes a node's rho (phi) by the rounding of its
    Q updates and of the Q-term sums that make the rest population: at most (Q + 2) half-ulps of values below the node's
    |rho| (1.01; |phi| <= 1), in every step; streaming moves values unchanged.  The bound lets that add up over every node
    and step."""
    dim, size, steps = 3, (32, 8, 8), 200
    ctrl = run(dim, size, steps, precision='single')
    t = _fe.make_twin(dim, size, np.float32)
    m0, p0 = float(t.f.astype(np.float64).sum()), float(t.g.astype(np.float64).sum())
    s = state(ctrl, dim)
    m1, p1 = float(s['f'].astype(np.float64).sum()), float(s['g'].astype(np.float64).sum())
    n, eps, Q = int(np.prod(size)), float(np.finfo(np.float32).eps), 19
    bound = n * steps * (Q + 2) * 0.5 * eps * 1.01
    print('mass drift %.3e, order parameter drift %.3e, bound %.3e' % (abs(m1 - m0), abs(p1 - p0), bound))
    assert np.all(np.isfinite(s['f'])) and np.all(np.isfinite(s['g']))
    assert abs(m1 - m0) <= bound and abs(p1 - p0) <= bound


# ---- refused again at module creation ---------------------------------------------------------------------------------------

MODULE_REFUSALS = [
    (dict(model=hipabi.SLF_MRT), 'mrt'),
    (dict(has_force=1, accel=[1e-5, 0, 0]), 'body forces'),
    (dict(type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_HALF_BB]), 'NTHalfBBWall'),
    (dict(type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_EQUILIBRIUM_DENSITY]), 'NTFullBBWall'),
    (dict(node_addressing=hipabi.SLF_ADDR_INDIRECT, dist_stride=4096), 'indirect'),
    (dict(incompressible=hipabi.SLF_DENSITY_INCOMPRESSIBLE), 'incompressible'),
    (dict(incompressible=hipabi.SLF_DENSITY_ROUNDOFF), 'minimize_roundoff'),
    (dict(regularized=1), 'regularized'),
    (dict(subgrid=hipabi.SLF_SUBGRID_LES_SMAGORINSKY, smagorinsky_const=0.1), 'subgrid'),
    (dict(bc_wall_grad_order=3), 'bc_wall_grad_order'),
]


@pytest.mark.parametrize('over,message', MODULE_REFUSALS, ids=[m for _, m in MODULE_REFUSALS])
def test_refused_at_module_creation(over, message):
    from sailfish_amd.backend_hip import HIPBackend, HIPFatalError

    class Opt(object):
        pass
    backend = HIPBackend(Opt(), 0)
    kw = dict(lattice=hipabi.SLF_D2Q9, model=hipabi.SLF_BGK, precision=8, access_pattern=hipabi.SLF_AB, lat_nx=18, lat_ny=10,
              arr_nx=32, arr_ny=10, tau=1.0, visc=1.0 / 6.0, tau_phi=1.0, simtype=hipabi.SLF_SIM_FREE_ENERGY, fluid_only=0,
              nt_type_mask=3, nt_misc_shift=2, type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_FULL_BB],
              fe_Gamma=0.5, fe_kappa=0.04, fe_A=0.04, fe_tau_a=1.0, fe_tau_b=1.0, bc_wall_grad_order=2)
    module = backend.build(hipabi.make_desc(**kw))
    with pytest.raises(HIPFatalError, match='CollideAndPropagate|single-fluid'):
        backend.get_kernel(module, 'CollideAndPropagate', None, [0] * 6 + [0], 'PPPPPPi')
    kw.update(over)
    with pytest.raises(HIPFatalError, match=message):
        backend.build(hipabi.make_desc(**kw))
