"""tests/_accf_twin.py, the numpy twin of a step with a per-node acceleration, held against the project's yardstick: with a
uniform field (and a zero uniform part, or the other way round) it is the CPU oracle's constant-force step bit for bit;
with a non-uniform field it adds the momentum sum(rho a) per step."""
import numpy as np
import pytest

from tests import _accf
from tests._accf_twin import AccfTwinBox, linear_field
from tests._oracle_box import OracleBox

SIZES = {'D2Q9': (13, 7), 'D3Q19': (9, 6, 5)}
ACCEL = [1.3e-5, -2.1e-5, 3.7e-5]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('force', ['guo', 'edm'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name', ['D2Q9', 'D3Q19'])
def test_uniform_field_is_the_oracles_constant_force(name, pattern, precision, force):
    grid, size = _accf.GRIDS[name], SIZES[name]
    dim = grid.dim
    accel = ACCEL[:dim]
    shape = tuple(reversed(size))
    for walls in (None, 'full', 'half'):
        for fused in ((1, 0) if walls is None else (1,)):
            d_o, periodic, map_fn = _accf.box_desc(grid, size, pattern, precision, force, walls, fused, accel=accel)
            oracle = _accf.start(OracleBox(d_o, periodic, None if map_fn is None else map_fn(d_o)), size, dim)
            twins = []
            for uniform, field in ((None, accel), (accel, [0.0] * dim)):
                d_t, _, _ = _accf.box_desc(grid, size, pattern, precision, force, walls, fused, accel=uniform, accel_field=True)
                assert d_t.accel_field == 1 and d_t.has_force == 1
                arrays = [np.full(shape, a) for a in field]
                twins.append(_accf.start(AccfTwinBox(d_t, periodic, None if map_fn is None else map_fn(d_t), accel_field=arrays),
                                         size, dim))
            for step in range(6):
                for s in [oracle] + twins:
                    s.step(save_macro=True)
                for t in twins:
                    what = (name, pattern, precision, force, walls, fused, step)
                    assert same(t.current_dist(), oracle.current_dist()), what
                    assert same(t.rho, oracle.rho), what
                    for k in range(dim):
                        assert same(t.v[k], oracle.v[k]), what
            assert np.all(np.isfinite(oracle.real_view(oracle.current_dist())))


def test_twin_without_a_field_is_the_oracle_too():
    """accel_field = 0: cp.accel alone (the code path the GPU tests never take, pinned here)."""
    grid, size = _accf.GRIDS['D2Q9'], SIZES['D2Q9']
    d, periodic, _ = _accf.box_desc(grid, size, 'AA', 'single', 'guo', accel=ACCEL[:2])
    o = _accf.start(OracleBox(d, periodic), size, 2)
    t = _accf.start(AccfTwinBox(d, periodic), size, 2)
    for s in (o, t):
        s.run(5)
    assert same(o.current_dist(), t.current_dist()) and same(o.rho, t.rho)


def momentum(grid, box):
    f = box.real_view(box.current_dist()).astype(np.float64)
    return np.array([sum(float(grid.basis[i][d]) * f[i].sum() for i in range(grid.Q)) for d in range(grid.dim)])


@pytest.mark.parametrize('force', ['guo', 'edm'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', ['D2Q9', 'D3Q19'])
def test_momentum_added_per_step(name, precision, force):
    """Fully periodic box, two-copy pattern: streaming conserves the total momentum and the collision adds rho a at every
    node (Guo: (1 - omega / 2) rho a from the source term + omega rho a / 2 from the shifted equilibrium; EDM: the
    difference of two equilibria), so P(t + 1) - P(t) = sum(rho(t) a).

    Tolerance: a post-collision population comes out of at most 16 rounded operations on values no larger than 2 |f_i|
    (the equilibrium polynomial, the relaxation, the source term), each off by at most eps / 2 of its result: 16 eps |f_i|.
    The momentum sums are formed in double precision from the stored values, |e_i| <= 1, sum_i |f_i| = rho, so
    |error| <= 16 eps sum(rho) per component -- worst case, every error in the same direction.  The field is of order 1e-3
    here, so that the bound (2e-6 of a population in single precision) stays three orders below what is added."""
    grid, size = _accf.GRIDS[name], SIZES[name]
    dim = grid.dim
    field = 100.0 * linear_field(size, dim)
    d, periodic, _ = _accf.box_desc(grid, size, 'AB', precision, force, accel_field=True)
    t = _accf.start(AccfTwinBox(d, periodic, accel_field=field), size, dim)
    eps = np.finfo(t.dtype).eps
    a = t.real_view(t.accel_field).astype(np.float64)             # as rounded to the format
    assert np.isnan(t.accel_field).sum() == t.accel_field.size - a.size      # padding and ghosts are NaN, never read
    for step in range(4):
        before = momentum(grid, t)
        rho = t.real_view(t.current_dist()).astype(np.float64).sum(axis=0)
        t.step()
        gained = momentum(grid, t) - before
        want = np.array([(rho * a[k]).sum() for k in range(dim)])
        tol = 16.0 * eps * rho.sum()
        print(name, precision, force, step, gained, want, np.abs(gained - want), tol)
        assert np.all(np.abs(want) > 100.0 * tol)
        assert np.all(np.abs(gained - want) <= tol)
