"""The numpy twin of the Tamm-Mott-Smith wall (tests/_tms_twin.py) on the CPU: against the values the reference's sympy
objects give (tests/golden/arith_tms_*.npz, tools/capture_tms.py), the property that makes the templates' target state the
paper's from the second step on, and a force-driven channel between TMS plates."""
import os

import numpy as np
import pytest

from sailfish_amd import sym
from tests import _tms_twin as tw

GRIDS = {'D2Q9': sym.D2Q9, 'D3Q19': sym.D3Q19}
FORMS = ['compressible', 'incompressible', 'roundoff']
KEYS = ('tg_rho', 'tg_v', 'repaired', 'rho', 'v', 'v_out', 'post')


def _wider(dtype):
    """The next wider format (tests/test_gpu_elbm.py): float64 for single; for double the x87 extended format where
    numpy has it."""
    if dtype is np.float32:
        return np.float64
    return np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else None


def _node(grid, f, missing, form, accel, visc, dtype):
    """tms_node() on the columns of f in `dtype`; lists of components become arrays [dim, n]."""
    tau = sym.relaxation_time(visc)
    r = tw.tms_node(grid, np.asarray(f, dtype=dtype), missing, form,
                    lambda g, rho, v, rho0: tw.bgk_collide(grid, g, rho, v, rho0, tau, accel, form))
    return {k: (np.array(r[k][:grid.dim]) if isinstance(r[k], list) else r[k]) for k in KEYS}


@pytest.mark.parametrize('force', ['none', 'guo'])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', sorted(GRIDS))
def test_twin_against_the_reference_expressions(golden_dir, name, form, force):
    """Every orientation and every link-tag word of the fixture, every state: the twin in float64 against the 30-digit
    values.  Tolerance per quantity: four times the largest difference between the twin in float64 and the twin in the
    next wider format on the same inputs (without a wider format: 16 eps, some 30 roundings of half an ulp of O(1) values
    per population)."""
    grid = GRIDS[name]
    G = np.load(os.path.join(golden_dir, 'arith_tms_%s.npz' % name))
    wts = np.array([float(w) for w in grid.weights])
    visc = float(G['visc'][0])
    missing = G['missing'].astype(bool).T                       # [Q, words]
    m = missing.shape[1]
    assert (G['use_tags'] == 0).sum() == 2 * grid.dim and (G['use_tags'] == 1).sum() == 3 ** grid.dim - 1
    # the words say what the masks say
    tags = G['use_tags'] == 1
    assert np.array_equal(tw.missing_from_tags(grid, G['words'][tags]), missing[:, tags])
    assert np.array_equal(tw.missing_from_orientation(grid, G['words'][~tags]), missing[:, ~tags])
    wide = _wider(np.float64)
    err = dict.fromkeys(KEYS, 0.0)
    tol = dict.fromkeys(KEYS, 0.0)
    for k in range(G['f'].shape[0]):
        fk = G['f'][k] - wts if form == 'roundoff' else G['f'][k]
        f = np.repeat(fk[:, None], m, axis=1)
        accel = list(G['accel'][k]) if force == 'guo' else None
        got = _node(grid, f, missing, form, accel, visc, np.float64)
        ref = _node(grid, f, missing, form, accel, visc, wide) if wide is not None else None
        for key in KEYS:
            want = np.moveaxis(G['%s_%s_%s' % (form, force, key)][:, k], 0, -1)         # [..., words]
            err[key] = max(err[key], float(np.max(np.abs(got[key] - want))))
            t = 16 * np.finfo(np.float64).eps if ref is None else float(np.max(np.abs(got[key] - ref[key])))
            tol[key] = max(tol[key], t)
    print({k: '%.2e / %.2e' % (err[k], 4 * tol[k]) for k in KEYS})
    for key in KEYS:
        assert err[key] <= 4 * tol[key], (key, err[key], tol[key])
    # the boundary condition does something: the repaired populations differ from the loaded ones exactly where missing
    rep = G['%s_none_repaired' % form][:, 0]                   # [words, Q]
    f0 = G['f'][0] - wts if form == 'roundoff' else G['f'][0]
    changed = rep != f0[None, :]
    unknown = np.zeros_like(changed)
    for i in range(1, grid.Q):
        unknown[:, grid.idx_opposite[i]] = G['missing'][:, i] == 1
    assert np.array_equal(changed, unknown)


def _random_populations(grid, lat, rng, dtype, roundoff=False):
    """rho in [0.9, 1.1], |u| <= 0.1 and a non-equilibrium part, on every node of the lattice (ghosts: 0)."""
    shape = tuple(lat)
    rho = rng.uniform(0.9, 1.1, shape)
    v = [rng.uniform(-0.1, 0.1, shape) / np.sqrt(grid.dim) for _ in range(grid.dim)] + [np.zeros(shape)] * (3 - grid.dim)
    f = tw.feq(grid, rho, rho, v) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (grid.Q,) + shape))
    if roundoff:
        f = f - np.array([float(w) for w in grid.weights]).reshape((grid.Q,) + (1,) * len(shape))
    real = np.zeros(shape, dtype=bool)
    real[tuple(slice(1, n - 1) for n in shape)] = True
    return np.where(real[None], f, 0.0).astype(dtype)


def plane_walls(grid, lat, axis):
    """TMS nodes on the first and the last real layer along lattice axis `axis` (0 = x), every other axis periodic.
    Returns (tms mask, link-tag words, orientation codes, periodic) over the lattice [(lat_nz,) lat_ny, lat_nx]."""
    nd = len(lat)
    k = nd - 1 - axis
    idx = np.indices(lat)[k]
    inside = np.ones(lat, dtype=bool)
    for a in range(nd):
        c = np.indices(lat)[a]
        inside &= (c >= 1) & (c <= lat[a] - 2)
    low, high = inside & (idx == 1), inside & (idx == lat[k] - 2)
    tags = np.zeros(lat, dtype=np.int64)
    orient = np.zeros(lat, dtype=np.int64)
    for i in range(1, grid.Q):
        e = grid.basis[i][axis]
        tags[low] |= (1 << (i - 1)) if e >= 0 else 0
        tags[high] |= (1 << (i - 1)) if e <= 0 else 0
    up = [0] * grid.dim
    up[axis] = 1
    orient[low] = grid.vec_to_dir(up)
    up[axis] = -1
    orient[high] = grid.vec_to_dir(up)
    periodic = [a != axis for a in range(grid.dim)]
    return low | high, tags, orient, periodic


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name,lat,axis', [('D2Q9', (6, 8), 1), ('D2Q9', (7, 6), 0), ('D3Q19', (5, 6, 7), 1),
                                           ('D3Q19', (6, 5, 6), 2)])
def test_loaded_unknowns_are_the_bounced_back_populations(name, lat, axis, pattern, form):
    """What settles the objection to the templates' target state: from the second step on, the populations a TMS node
    loads in its unknown slots are the opposite post-collision populations of its own previous step -- exactly, under both
    access patterns, with link tags and with orientation codes -- so (tg_rho, tg_v) is the state after bounce-back, the
    paper's.  Only the first step after hand-set populations differs."""
    grid = GRIDS[name]
    rng = np.random.RandomState(7)
    f0 = _random_populations(grid, lat, rng, np.float64, form == 'roundoff')
    tms, tags, orient, periodic = plane_walls(grid, lat, axis)
    opp = grid.idx_opposite
    for missing in (tw.missing_from_tags(grid, tags), tw.missing_from_orientation(grid, orient)):
        t = tw.TmsTwin(grid, f0, tms, missing, 0.02, periodic, pattern=pattern, density=form, accel=[1e-5, 0.0, 2e-5][:grid.dim])
        assert t.missing.any()
        t.step()
        for step in range(1, 5):
            prev = t.post.copy()
            t.step()
            for i in range(1, grid.Q):
                mi = t.missing[i]
                assert np.array_equal(t.loaded[opp[i]][mi], prev[i][mi]), (step, i)
        assert np.isfinite(t.current()).all()


def _steady_channel(pattern, form, ny=12, steps=4000):
    grid = sym.D2Q9
    lat = (ny + 2, 6)                                      # (lat_ny, lat_nx): 4 real columns, periodic
    tms, tags, _, periodic = plane_walls(grid, lat, 1)
    rho = np.ones(lat)
    zero = np.zeros(lat)
    f = tw.feq(grid, rho, rho, [zero, zero, zero])
    if form == 'roundoff':
        f = f - np.array([float(w) for w in grid.weights]).reshape(grid.Q, 1, 1)
    visc, g = 1.0 / 6.0, 1e-6
    t = tw.TmsTwin(grid, f, tms, tw.missing_from_tags(grid, tags), visc, periodic, pattern=pattern, density=form,
                   accel=[g, 0.0])
    t.run(steps)
    return t, visc, g


@pytest.mark.parametrize('form', ['compressible', 'roundoff'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_force_driven_channel_between_tms_plates(pattern, form):
    """A body force along x between two TMS plates, run to a steady state (4000 steps = 4.6 diffusion times H^2 / nu of
    the 12-node channel).  The profile is symmetric about the centre line and the wall-normal velocity vanishes, both to
    rounding -- one rounding of an O(1) population per step, eps per step, added up over every step without any damping --
    and the velocity falls monotonically towards the walls.  The effective wall position the parabola through the
    profile gives is printed (and recorded in DESIGN.md), not asserted."""
    steps = 4000
    t, visc, g = _steady_channel(pattern, form, steps=steps)
    ux = t.v[0][1:-1, 1:-1]
    uy = t.v[1][1:-1, 1:-1]
    ny = ux.shape[0]
    bound = steps * np.finfo(np.float64).eps
    assert np.max(np.abs(ux - ux[:, :1])) <= bound                    # uniform along x
    u = ux[:, 0]
    assert u.min() > 0
    assert np.max(np.abs(u - u[::-1])) <= bound
    assert np.max(np.abs(uy)) <= bound
    half = u[:ny // 2 + 1] if ny % 2 else u[:ny // 2]
    assert np.all(np.diff(half) > 0)
    # steady: the last 200 steps change the profile by less than 1e-6 of its maximum
    before = u.copy()
    t.run(200)
    assert np.max(np.abs(t.v[0][1:-1, 1] - before)) <= 1e-6 * u.max()
    # u(y) = g / (2 nu) (y - y_w) (y_top - y): the wall position from a parabola through the node values
    y = np.arange(ny, dtype=np.float64)
    c2, c1, c0 = np.polyfit(y, u, 2)
    roots = np.sort(np.roots([c2, c1, c0]).real)
    print('%s %s: curvature %.6e (g / 2 nu = %.6e), walls at %.4f and %.4f node spacings outside the first / last node'
          % (pattern, form, -c2, g / (2 * visc), -roots[0], roots[1] - (ny - 1)))
