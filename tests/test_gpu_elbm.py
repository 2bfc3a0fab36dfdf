"""The entropic collision (--model=elbm) on the GPU, against its numpy twin (tests/_elbm_twin.py, itself held against the
reference's sympy objects by tests/test_elbm_twin.py) and against itself across configurations.  Tolerances are sized
from the twin and from the number formats, never from what the kernels return; properties of the Newton solution are
checked on the host in float64 from the alpha the device stored.  No test depends on making the solver fail."""
import os

import numpy as np
import pytest

from sailfish_amd import hipabi, lb_single, sym
from sailfish_amd.box import BoxSim, make_box_desc
from tests import _elbm_twin as tw
from tests import _geometry as geo
from tests.test_elbm_twin import SHEAR, kinetic_energy, shear_layer

pytestmark = pytest.mark.gpu

GRIDS = {'D2Q9': (sym.D2Q9, (66, 5)), 'D3Q19': (sym.D3Q19, (64, 4, 3))}
DTYPE = {'single': np.float32, 'double': np.float64}
EQUILIBRIA = [False, True]
VISC = 0.01


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def _wider(dtype):
    """The next wider format, for the twin's own rounding error: float64 for single; for double the x87 extended format
    where numpy has it."""
    if dtype is np.float32:
        return np.float64
    return np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else None


def _twin_error(grid, f, dtype, ent, keys=('alpha', 'f')):
    """Largest difference between the twin in `dtype` and the twin in the next wider format over the states f [Q, n]."""
    r = tw.collide(grid, f.astype(dtype), VISC, entropic_eq=ent)
    wide = _wider(dtype)
    if wide is None:         # no wider format: a collision is some 20 roundings per population, each of half an ulp of O(1)
        return r, {k: 16 * np.finfo(dtype).eps for k in keys}
    # the same inputs (already rounded to dtype), wider arithmetic
    w = tw.collide(grid, f.astype(dtype).astype(wide), VISC, entropic_eq=ent)
    return r, {k: float(np.max(np.abs(r[k].astype(wide) - w[k]))) for k in keys}


class _StateBox(object):
    """A periodic box every node of which carries the same populations: invariant under streaming, so one step leaves
    each node with the post-collision state (the device of tests/test_gpu_reg_les.py)."""

    def __init__(self, backend, grid, size, precision, ent, alpha_field=True):
        desc = make_box_desc(grid, size, model='elbm', precision=precision, access_pattern='AB', visc=VISC,
                             periodic_fused=[1] * 3, entropic_equilibrium=ent)
        self.s = BoxSim(backend, desc, periodic=(True, True, True), alpha_field=alpha_field)

    def step(self, f, alpha0=2.0):
        s = self.s
        full = np.empty((s.Q,) + s.shape, dtype=s.dtype)
        full[...] = np.asarray(f, dtype=s.dtype).reshape((s.Q,) + (1,) * len(s.shape))
        s.set_dist(full)
        if s.gpu_alpha is not None:
            s.set_alpha(alpha0)
        s.step(save_macro=False)
        out = s.real_view(s.get_dist()).reshape(s.Q, -1)
        assert np.all(out == out[:, :1])                       # every node did the same arithmetic
        assert s.backend.poll_invalid(s.module, s.stream) is None
        alpha = None
        if s.gpu_alpha is not None:
            a = s.real_view(s.fetch_alpha()).reshape(-1)
            assert np.all(a == a[0])
            alpha = a[0]
        return out[:, 0].copy(), alpha


@pytest.mark.parametrize('ent', EQUILIBRIA, ids=['polynomial', 'product'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', sorted(GRIDS))
def test_small_deviation_and_series_regimes(backend, golden_dir, name, precision, ent):
    grid, size = GRIDS[name]
    G = np.load(os.path.join(golden_dir, 'arith_elbm_%s.npz' % name))
    key = 'entropic' if ent else 'bgk'
    dtype = DTYPE[precision]
    sel = G['regime_' + key] < 2
    f = G['f_' + key][sel].T
    r, tol = _twin_error(grid, f, dtype, ent)
    assert np.array_equal(r['regime'], G['regime_' + key][sel]) and (r['regime'] == 1).sum() >= 8
    box = _StateBox(backend, grid, size, precision, ent)
    err = {'alpha': 0.0, 'f': 0.0}
    for k in range(f.shape[1]):
        out, alpha = box.step(f[:, k])
        err['alpha'] = max(err['alpha'], abs(float(alpha) - float(r['alpha'][k])))
        err['f'] = max(err['f'], float(np.max(np.abs(out.astype(np.float64) - r['f'][:, k].astype(np.float64)))))
    print('%s %s %s: |alpha - twin| %.3e (tol %.3e), |f - twin| %.3e (tol %.3e)'
          % (name, precision, key, err['alpha'], 4 * tol['alpha'], err['f'], 4 * tol['f']))
    assert err['alpha'] <= 4 * tol['alpha'] and err['f'] <= 4 * tol['f'], (err, tol)


@pytest.mark.parametrize('ent', EQUILIBRIA, ids=['polynomial', 'product'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', sorted(GRIDS))
def test_newton_regime(backend, golden_dir, name, precision, ent):
    """What the stop rule promises, for the alpha the device stored: the entropy equality within the tolerance plus the
    rounding of two Q-term sums in the kernel's precision, 1 <= alpha <= max_alpha, and populations relaxed with exactly
    that alpha.  Cold (alpha field at 2) and warm-started from the previous answer; and without an alpha array."""
    grid, size = GRIDS[name]
    G = np.load(os.path.join(golden_dir, 'arith_elbm_%s.npz' % name))
    key = 'entropic' if ent else 'bgk'
    dtype = DTYPE[precision]
    R = dtype
    eps = float(np.finfo(dtype).eps)
    f = G['f_' + key][G['regime_' + key] == 2].T.astype(dtype)
    small = G['f_' + key][G['regime_' + key] < 2].T
    _, tol = _twin_error(grid, small, dtype, ent)                 # the regime-1 tolerance
    twin = tw.collide(grid, f, VISC, entropic_eq=ent)                 # fneq as the kernel forms it, in its precision
    assert np.all(twin['regime'] == 2)
    etol = tw.default_entropy_tolerance(dtype)
    ln_w = np.log(np.array([float(w) for w in grid.entropic_weights]))
    beta = tw.beta_of(VISC, R)
    box = _StateBox(backend, grid, size, precision, ent)
    bare = _StateBox(backend, grid, size, precision, ent, alpha_field=False)
    worst = 0.0
    for k in range(f.shape[1]):
        fk, fneq = f[:, k], twin['fneq'][:, k]
        f64, fneq64 = fk.astype(np.float64), fneq.astype(np.float64)
        h0_terms = f64 * (np.log(f64) - ln_w)
        bound = etol + 2 * (grid.Q + 4) * eps * np.abs(h0_terms).sum()
        amax = float(tw.max_alpha(fk[:, None], fneq[:, None])[0])
        start = 2.0
        for attempt in ('cold', 'warm'):
            out, alpha = box.step(fk, start)
            fa = f64 + float(alpha) * fneq64
            dh = abs(float((fa * (np.log(fa) - ln_w)).sum() - h0_terms.sum()))
            worst = max(worst, dh / bound)
            assert dh <= bound, (attempt, k, dh, bound, float(alpha))
            assert 1.0 <= alpha <= amax, (attempt, k, float(alpha), amax)
            want = fk + (R(alpha) * beta) * fneq
            assert np.max(np.abs(out.astype(np.float64) - want.astype(np.float64))) <= 4 * tol['f'], (attempt, k)
            if attempt == 'warm':
                assert abs(float(alpha) - start) < 1e-3
            start = float(alpha)
        out, none = bare.step(fk)
        assert none is None
        # no array: the cold start; the same arithmetic, the same bits as the cold run above
        cold, _ = box.step(fk, 2.0)
        assert np.array_equal(out, cold)
    print('%s %s %s: worst |dH| / bound %.3f' % (name, precision, key, worst))


def _perturbed_fields(size, dim, amp=0.03):
    idx = np.meshgrid(*[np.arange(n) for n in reversed(size)], indexing='ij')
    phase = sum((k + 1) * 2 * np.pi * c / n for k, (c, n) in enumerate(zip(idx, reversed(size))))
    rho = 1.0 + 0.02 * np.sin(phase)
    v = [amp * np.sin(phase + 1.3 * d) * np.cos(2 * np.pi * idx[d % dim] / idx[d % dim].shape[d % dim] + d)
         for d in range(dim)]
    return rho, v


def _moments64(grid, f):
    f = np.asarray(f, dtype=np.float64).reshape(grid.Q, -1)
    e = np.array(grid.basis, dtype=np.float64)
    return f.sum(), e.T.dot(f.sum(axis=1))


@pytest.mark.parametrize('ent', EQUILIBRIA, ids=['polynomial', 'product'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('grid,size', [(sym.D2Q9, (64, 24)), (sym.D3Q19, (64, 8, 6))], ids=['D2Q9', 'D3Q19'])
def test_conservation(backend, grid, size, precision, ent):
    """50 steps on a perturbed periodic box.  A collision changes the mass of a node by the rounding of its Q updates and
    of the Q-term sum of fneq, at most (Q / 2 + 1) ulp of its density; the bound lets that add up over every node and
    step.  Momentum likewise (the errors scale with the populations, not with the velocity) with the polynomial
    equilibrium; the product form does not conserve momentum exactly (D3Q19: a series truncated at order 8) -- there the
    bound is four times what the twin shows on the same run."""
    steps, dtype = 50, DTYPE[precision]
    rho, v = _perturbed_fields(size, grid.dim)
    t = tw.ElbmTwin.from_fields(grid, rho, v, VISC, dtype=dtype, entropic_eq=ent)
    desc = make_box_desc(grid, size, model='elbm', precision=precision, access_pattern='AB', visc=VISC,
                         periodic_fused=[1] * 3, entropic_equilibrium=ent)
    s = BoxSim(backend, desc, periodic=(True, True, True))
    full = np.zeros((s.Q,) + s.shape, dtype=s.dtype)
    s.real_view(full)[...] = t.f
    s.set_dist(full)
    m0, p0 = _moments64(grid, t.f)
    s.run(steps, save_last=True)
    assert s.backend.poll_invalid(s.module, s.stream) is None
    m1, p1 = _moments64(grid, s.real_view(s.get_dist()))
    t.run(steps)
    assert t.failed == 0
    _, pt = _moments64(grid, t.f)
    rounding = steps * (grid.Q / 2.0 + 1) * float(np.finfo(dtype).eps) * m0
    drift = float(np.max(np.abs(p1 - p0)))
    twin_drift = float(np.max(np.abs(pt - p0)))
    print('%s %s product=%s: mass %.3e, momentum %.3e, twin momentum %.3e, rounding bound %.3e'
          % (grid.__name__, precision, ent, abs(m1 - m0), drift, twin_drift, rounding))
    assert abs(m1 - m0) <= rounding
    assert drift <= (4 * twin_drift if ent else rounding)
    s.release()


# ---- bit-identical between configurations of the same build ---------------------------------------------------------

def _cavity_classes():
    from examples.ldc_2d import CavitySubdomain as Cavity2D
    from examples.ldc_3d import CavitySubdomain as Cavity3D

    class Sim2D(lb_single.LBEntropicFluidSim):
        subdomain = Cavity2D

    class Sim3D(lb_single.LBEntropicFluidSim):
        subdomain = Cavity3D
    return {2: Sim2D, 3: Sim3D}


CAVITY = {2: dict(lat_nx=40, lat_ny=30, visc=0.002), 3: dict(lat_nx=24, lat_ny=14, lat_nz=12, visc=0.002, grid='D3Q19')}


def _run_cavity(dim, steps, precision, ent, **kw):
    from tests.test_gpu_runner import merged_gpu, run_gpu
    cfg = dict(CAVITY[dim], precision=precision, entropic_equilibrium=ent)
    extra = kw.pop('extra', None)
    cfg.update(kw)
    ctrl = run_gpu(_cavity_classes()[dim], None, dim, cfg, steps, extra=extra)
    out = {'dist': merged_gpu(ctrl, 'dist'), 'rho': merged_gpu(ctrl, 'rho')}
    for d in range(dim):
        out['v%d' % d] = merged_gpu(ctrl, 'v%d' % d)
    r0 = ctrl.runners[0]
    alpha = np.zeros(tuple(reversed(r0._global_size)), dtype=r0.float)
    for r in ctrl.runners:
        sl = tuple(slice(o, o + n) for o, n in zip(reversed(r._spec.location), reversed(r._spec.size)))
        alpha[sl] = r._sim.alpha
    out['alpha'] = alpha
    return out


def _same(a, b, populations=True):
    """Fields (the moments the last step read, and its alpha) and, where both runs keep them in the same layout, the
    populations.  The in-place pattern stores the populations of a step in a layout of its own, and indirect addressing
    gives no slot to nodes that are not active: there the fields are compared."""
    for key in sorted(a):
        if key != 'dist' or populations:
            assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert np.ptp(a['alpha']) > 0 and np.ptp(a['v0']) > 0


@pytest.mark.parametrize('ent', EQUILIBRIA, ids=['polynomial', 'product'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('steps', [40, 41])
def test_configurations_agree_bit_for_bit(dim, steps, precision, ent):
    """-ffp-contract=off and a node-local alpha: the access pattern, the addressing mode and the decomposition change
    where the numbers live, not the numbers."""
    base = _run_cavity(dim, steps, precision, ent, access_pattern='AB')
    in_place = _run_cavity(dim, steps, precision, ent, access_pattern='AA')
    _same(base, in_place, populations=False)
    _same(base, _run_cavity(dim, steps, precision, ent, access_pattern='AB', node_addressing='indirect'), populations=False)
    _same(in_place, _run_cavity(dim, steps, precision, ent, access_pattern='AA', node_addressing='indirect'), populations=False)
    for nsub, axis in [(2, 'x'), (3, 'x')] + ([(2, 'z'), (3, 'z')] if dim == 3 else [(2, 'y'), (3, 'y')]):
        _same(base, _run_cavity(dim, steps, precision, ent, access_pattern='AB', subdomains=nsub, conn_axis=axis))
        _same(in_place, _run_cavity(dim, steps, precision, ent, access_pattern='AA', subdomains=nsub, conn_axis=axis))


@pytest.mark.parametrize('ent', EQUILIBRIA, ids=['polynomial', 'product'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('dim,pattern', [(2, 'AB'), (3, 'AA')])
def test_checkpoint_and_restore(dim, pattern, precision, ent, tmp_path):
    """A run interrupted at step 24 and restored equals the uninterrupted one: the alpha field travels with the
    checkpoint, so the Newton iterations of step 25 start where they would have."""
    straight = _run_cavity(dim, 41, precision, ent, access_pattern=pattern)
    ck = str(tmp_path / 'ck')
    _run_cavity(dim, 24, precision, ent, access_pattern=pattern, extra=dict(checkpoint_file=ck, final_checkpoint=True))
    cp = [f for f in os.listdir(str(tmp_path)) if f.endswith('.cpoint.npz')]
    assert len(cp) == 1 and 'field_alpha' in np.load(os.path.join(str(tmp_path), cp[0])).files
    resumed = _run_cavity(dim, 41, precision, ent, access_pattern=pattern,
                          extra=dict(restore_from=os.path.join(str(tmp_path), cp[0][:-len('.0.cpoint.npz')])))
    _same(straight, resumed)


# ---- against the twin over time -------------------------------------------------------------------------------------

def _closed_box(desc, dim):
    """Full-way bounce-back walls all around (the twin's boundary condition)."""
    m = geo.empty_map(desc)
    w = geo.encode(geo.T_FULLBB)
    ny, nx = desc.lat_ny - 2, desc.lat_nx - 2
    if dim == 2:
        m[0, 1, 1:nx + 1] = m[0, ny, 1:nx + 1] = w
        m[0, 1:ny + 1, 1] = m[0, 1:ny + 1, nx] = w
    else:
        nz = desc.lat_nz - 2
        m[1, 1:ny + 1, 1:nx + 1] = m[nz, 1:ny + 1, 1:nx + 1] = w
        m[1:nz + 1, 1, 1:nx + 1] = m[1:nz + 1, ny, 1:nx + 1] = w
        m[1:nz + 1, 1:ny + 1, 1] = m[1:nz + 1, 1:ny + 1, nx] = w
    return m


@pytest.mark.parametrize('ent', EQUILIBRIA, ids=['polynomial', 'product'])
@pytest.mark.parametrize('case', ['periodic', 'cavity'])
@pytest.mark.parametrize('grid,size', [(sym.D2Q9, (40, 24)), (sym.D3Q19, (32, 10, 8))], ids=['D2Q9', 'D3Q19'])
def test_twenty_steps_against_the_twin(backend, grid, size, case, ent):
    """Double precision, 20 steps, a flow strong enough for the Newton branch.  Two equally valid implementations of the
    collision -- the twin with ln x and the twin with log2(x) ln 2 -- drift apart by `spread`; the kernels may be 100
    times that from the twin (floor: 1e-13 relative).  `cavity`: a closed box of full-way bounce-back walls around a
    stirred fluid -- the boundary condition the twin has (the lid of the examples is a regularized-velocity node)."""
    steps, visc = 20, 0.002
    rho, v = _perturbed_fields(size, grid.dim, amp=0.08)
    kw = dict(model='elbm', precision='double', access_pattern='AB', visc=visc, entropic_equilibrium=ent)
    if case == 'periodic':
        desc = make_box_desc(grid, size, periodic_fused=[1] * 3, **kw)
        s = BoxSim(backend, desc, periodic=(True, True, True))
        wall = None
    else:
        desc = make_box_desc(grid, size, fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, **kw)
        node_map = _closed_box(desc, grid.dim)
        s = BoxSim(backend, desc, node_map=node_map)
        wall = s.real_view(node_map) == geo.encode(geo.T_FULLBB)
    twins = [tw.ElbmTwin.from_fields(grid, rho, v, visc, wall=wall, entropic_eq=ent, log2=l2) for l2 in (False, True)]
    full = np.zeros((s.Q,) + s.shape, dtype=s.dtype)
    s.real_view(full)[...] = twins[0].f
    for which in range(len(s.gpu_dist)):
        s.set_dist(full, which)
    s.run(steps, save_last=True)
    assert s.backend.poll_invalid(s.module, s.stream) is None
    for t in twins:
        t.run(steps)
        assert t.failed == 0
    assert twins[0].regime_counts[2] > 0
    fluid = np.ones(twins[0].shape, dtype=bool) if wall is None else ~wall
    got = s.real_view(s.get_dist())[:, fluid]
    ref = twins[0].f[:, fluid]
    scale = float(np.max(np.abs(ref)))
    spread = float(np.max(np.abs(twins[1].f[:, fluid] - ref))) / scale
    err = float(np.max(np.abs(got - ref))) / scale
    tol = max(100 * spread, 1e-13)
    assert err <= tol, 'kernels vs twin %.3e relative; spread between the two twins %.3e (tolerance %.3e)' % (err, spread, tol)
    s.release()


# ---- the reason the model exists ------------------------------------------------------------------------------------

def test_under_resolved_shear_layer(backend):
    """A doubly periodic shear layer two nodes thick at Re = 10^4 on 64 x 64 nodes, single precision; viscosity and step
    count are the ones tests/test_elbm_twin.py shows the twin gets through."""
    n = SHEAR['n']
    rho, v = shear_layer(**SHEAR)
    desc = make_box_desc(sym.D2Q9, (n, n), model='elbm', precision='single', access_pattern='AA', visc=SHEAR['visc'],
                         periodic_fused=[1] * 3)
    s = BoxSim(backend, desc, periodic=(True, True, True))
    s.set_fields(rho, v)
    s.initial_conditions()
    k0 = kinetic_energy(rho, v)
    s.run(SHEAR['steps'], save_last=True)
    assert s.backend.poll_invalid(s.module, s.stream) is None
    assert np.isfinite(s.real_view(s.get_dist())).all()
    g_rho, g_v = s.fetch_fields()
    k1 = kinetic_energy(s.real_view(g_rho), [s.real_view(c) for c in g_v])
    alpha = s.real_view(s.fetch_alpha())
    print('kinetic energy %.6f of the initial; alpha in [%.4f, %.4f]' % (k1 / k0, alpha.min(), alpha.max()))
    assert k1 <= k0
    assert np.any(alpha != 2.0)
    assert np.all(alpha >= 1.0)
    s.release()


# ---- what the library refuses ---------------------------------------------------------------------------------------

def _desc(**kw):
    args = dict(precision='single', access_pattern='AB', visc=0.01, periodic_fused=[1, 1, 1], model='elbm')
    args.update(kw)
    return make_box_desc(sym.D3Q19, (16, 4, 4), **args)


def test_refusals(backend):
    def refused(desc, message):
        with pytest.raises(backend.FatalError, match=message):
            backend.build(desc)

    backend.build(_desc())
    backend.build(_desc(incompressible=True))
    d = _desc()
    for i, r in enumerate(sym.mrt_rates(sym.D3Q19, 0.01)):
        d.mrt_rates[i] = r
    refused(d, 'MRT relaxation rates')
    refused(_desc(regularized=True), 'regularized / subgrid: --model=elbm is not served; --model=bgk only')
    refused(_desc(subgrid=True), 'regularized / subgrid: --model=elbm is not served; --model=bgk only')
    for simtype in (hipabi.SLF_SIM_SHAN_CHEN_BINARY, hipabi.SLF_SIM_SHAN_CHEN_SINGLE):
        d = _desc()
        d.simtype = simtype
        d.tau_phi = 1.0
        refused(d, 'single-fluid modules only')
    refused(_desc(incompressible=hipabi.SLF_DENSITY_ROUNDOFF), 'minimize_roundoff')
    refused(_desc(incompressible=True, entropic_equilibrium=True), 'not with the incompressible')
    refused(_desc(accel=[1e-5, 0.0, 0.0]), 'body forces')
    refused(_desc(model='bgk', entropic_equilibrium=True), 'entropic_equilibrium needs model')
    refused(_desc(model='mrt', entropic_equilibrium=True), 'entropic_equilibrium needs model')
    d = _desc()
    d.entropy_tolerance = 0.0
    refused(d, 'entropy_tolerance')
    # the resident several-steps kernel does not serve the model
    d2 = make_box_desc(sym.D2Q9, (32, 32), model='elbm', precision='single', access_pattern='AB', periodic_fused=[1, 1, 1])
    m = backend.build(d2)
    with pytest.raises(backend.FatalError, match='CollideAndPropagateResident'):
        backend.get_kernel(m, 'CollideAndPropagateResident', (64,), [0, 1, 2, 3, 4, 0, 2, 8, 8, 3], 'PPPPPiiiii',
                           needs_iteration=True)
