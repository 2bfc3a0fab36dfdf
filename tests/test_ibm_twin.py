"""tests/_ibm_twin.py, the numpy twin of a step with immersed boundary markers, held against what it is
composed of and against the identities the method rests on.  No GPU."""
import numpy as np
import pytest

from tests import _accf
from tests._accf_twin import AccfTwinBox
from tests._ibm_twin import SCALE, IbmTwinBox

SIZES = {'D2Q9': (13, 7), 'D3Q19': (9, 6, 5)}


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def markers(size, n, seed=3, margin=1.0):
    """n positions well inside the box of real nodes (global coordinates 0 .. size - 1), reference positions next to them."""
    rng = np.random.RandomState(seed)
    hi = np.array(size, dtype=np.float64) - 1.0 - margin
    pos = margin + rng.rand(n, len(size)) * (hi - margin)
    ref = pos + 0.8 * (rng.rand(n, len(size)) - 0.5)
    return pos, ref


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name', ['D2Q9', 'D3Q19'])
def test_without_stiffness_the_twin_is_the_field_twin_with_a_zero_field(name, pattern, precision):
    grid, size = _accf.GRIDS[name], SIZES[name]
    dim = grid.dim
    shape = tuple(reversed(size))
    pos, ref = markers(size, 9)
    for walls in (None, 'full'):
        desc, periodic, map_fn = _accf.box_desc(grid, size, pattern, precision, 'guo', walls, accel=[1e-5, -2e-5, 3e-5][:dim],
                                                accel_field=True)
        nmap = None if map_fn is None else map_fn(desc)
        plain = _accf.start(AccfTwinBox(desc, periodic, nmap, accel_field=np.zeros((dim,) + shape)), size, dim)
        ibm = _accf.start(IbmTwinBox(desc, periodic, nmap, pos, ref, np.zeros(9)), size, dim)
        for step in range(5):
            plain.step(save_macro=True)
            ibm.step()
            assert same(ibm.current_dist(), plain.current_dist()), (walls, step)
            assert same(ibm.rho, plain.rho) and all(same(a, b) for a, b in zip(ibm.v, plain.v)), (walls, step)
            assert same(ibm.accel_field, plain.accel_field) and not ibm.acc.any()
        assert not same(ibm.positions(), pos.astype(ibm.dtype))          # the markers did move with the fluid
        assert ibm.outside == 0


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', ['D2Q9', 'D3Q19'])
def test_accumulator_sum_is_the_sum_of_the_quantised_contributions(name, precision):
    grid, size = _accf.GRIDS[name], SIZES[name]
    dim = grid.dim
    pos, ref = markers(size, 40)
    pos[10:25] = pos[10]                      # contention: fifteen markers on the same nodes
    desc, periodic, _ = _accf.box_desc(grid, size, 'AB', precision, 'guo', accel_field=True)
    t = IbmTwinBox(desc, periodic, None, pos, ref, np.linspace(0.01, 0.3, 40))
    t.spread()
    assert len(t.quantised) == dim * 2 ** dim
    for k in range(dim):
        want = sum(int(x) for kk, q in t.quantised if kk == k for x in q)
        assert int(t.acc[k].sum(dtype=object)) == want and want != 0
    # and the field is the accumulator, scaled back, at the stencil nodes and nowhere else
    t.gather()
    real = t.real_view(t.accel_field)
    assert np.array_equal(real != 0, t.real_view(t.acc) != 0)
    assert np.array_equal(real, (t.real_view(t.acc).astype(np.float64) / SCALE).astype(t.dtype))


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', ['D2Q9', 'D3Q19'])
def test_weights_at_integer_coordinates_are_one_and_zero(name, precision):
    grid, size = _accf.GRIDS[name], SIZES[name]
    dim = grid.dim
    desc, periodic, _ = _accf.box_desc(grid, size, 'AB', precision, 'guo', accel_field=True)
    t = IbmTwinBox(desc, periodic, None, [[3.0, 2.0, 1.0][:dim]], [[3.0, 2.0, 1.0][:dim]], [1.0])
    nodes, inside = t.stencil()
    assert inside.all() and len(nodes) == 2 ** dim
    assert [float(w[0]) for _, _, w in nodes] == [1.0] + [0.0] * (2 ** dim - 1)
    valid, idx, _ = nodes[0]
    assert valid.all() and [int(c[0]) for c in idx] == [(1 + 1) if dim == 3 else 0, 2 + 1, 3 + 1]       # array index = coordinate + 1


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', ['D2Q9', 'D3Q19'])
def test_linear_velocity_field_is_interpolated_exactly_up_to_rounding(name, precision):
    """v = a + b . x at the nodes gives a + b . x_p at the marker.  Bound, relative to the largest |v| of a node: a weight
    factor 1 - |x - i| is off by at most eps of itself (the difference, where it is not exact, and the subtraction from
    one), the product of dim factors and v adds dim roundings of eps / 2, the 2^dim - 1 additions eps / 2 each of a
    partial sum no larger than max |v|: (1.5 dim + 2^(dim - 1)) eps, asserted with a factor of two as (3 dim + 2^dim) eps.
    The measured maximum is printed."""
    grid, size = _accf.GRIDS[name], SIZES[name]
    dim = grid.dim
    pos, _ = markers(size, 64, seed=8)
    desc, periodic, _ = _accf.box_desc(grid, size, 'AB', precision, 'guo', accel_field=True)
    t = IbmTwinBox(desc, periodic, None, pos, pos, np.zeros(64))
    a = np.array([0.01, -0.02, 0.015])[:dim]
    b = np.array([[1e-3, -2e-3, 3e-3], [2.5e-3, 1.5e-3, -1e-3], [-3e-3, 1e-3, 2e-3]])[:dim, :dim]
    coords = np.indices(tuple(reversed(size))).astype(np.float64)[::-1]              # x, y[, z] of the real nodes
    for k in range(dim):
        t.real_view(t.v[k])[...] = a[k] + sum(b[k][j] * coords[j] for j in range(dim))
    nodes = [t.real_view(t.v[k]).astype(np.float64) for k in range(dim)]            # as rounded to the format
    start = t.pos.astype(np.float64)
    t.clear_and_advect()
    eps = np.finfo(t.dtype).eps
    worst = 0.0
    for k in range(dim):
        # the linear function through the ROUNDED node values is not linear any more: compare with the exact multilinear
        # interpolant of the stored values at the stored positions, formed in float64
        want = np.zeros(64)
        i0 = np.floor(start).astype(int)
        for corner in np.ndindex(*([2] * dim)):
            w = np.ones(64)
            for j in range(dim):
                w = w * (1.0 - np.abs(start[j] - (i0[j] + corner[j])))
            want += w * nodes[k][tuple(i0[j] + corner[j] for j in reversed(range(dim)))]
        err = np.abs(t.last_vp[k].astype(np.float64) - want).max() / np.abs(nodes[k]).max()
        worst = max(worst, err)
        # and that interpolant is the linear function itself up to the rounding of the node values (eps / 2 each, weights
        # that sum to one) and the float64 arithmetic of the two expressions compared here (2^dim + dim operations each)
        exact = a[k] + sum(b[k][j] * start[j] for j in range(dim))
        assert np.abs(want - exact).max() <= (eps / 2 + 2 * (2 ** dim + dim) * np.finfo(np.float64).eps) * np.abs(nodes[k]).max()
    bound = (3 * dim + 2 ** dim) * eps
    print('%s %s: interpolation error %.3e of max |v|, bound %.3e' % (name, precision, worst, bound))
    assert worst <= bound


def momentum(grid, box):
    f = box.real_view(box.current_dist()).astype(np.float64)
    return np.array([sum(float(grid.basis[i][d]) * f[i].sum() for i in range(grid.Q)) for d in range(grid.dim)])


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', ['D2Q9', 'D3Q19'])
def test_displaced_markers_feed_momentum_into_a_fluid_at_rest(name, precision):
    """The identity of tests/test_accf_twin.py with the field the markers make: in a periodic two-copy box
    P(t + 1) - P(t) = sum(rho(t) a), a the field after gather; |error| <= 16 eps sum(rho) (derived there).  And the
    field is the springs': sum(a[d]) = sum over the markers of -k (x[d] - ref[d]) times the sum of the weights, 1."""
    grid, size = _accf.GRIDS[name], SIZES[name]
    dim = grid.dim
    pos, _ = markers(size, 6, seed=5, margin=2.0)
    ref = pos + np.array([1.5, -1.0, 0.7])[:dim]
    k = np.full(6, 0.05)
    desc, periodic, _ = _accf.box_desc(grid, size, 'AB', precision, 'guo', accel_field=True)
    t = IbmTwinBox(desc, periodic, None, pos, ref, k)
    t.set_fields(np.ones(tuple(reversed(size))), [np.zeros(tuple(reversed(size)))] * dim)
    t.initial_conditions()
    eps = np.finfo(t.dtype).eps
    for step in range(3):
        t.spread()
        t.gather()
        a = t.real_view(t.accel_field).astype(np.float64)
        pull = (-t.k.astype(np.float64)) * (t.pos.astype(np.float64) - t.ref.astype(np.float64))
        assert np.allclose(a.reshape(dim, -1).sum(axis=1), pull.sum(axis=1), rtol=64 * eps, atol=6 * 2 ** dim / SCALE)
        before = momentum(grid, t)
        rho = t.real_view(t.current_dist()).astype(np.float64).sum(axis=0)
        AccfTwinBox.step(t, save_macro=True)
        gained = momentum(grid, t) - before
        t.clear_and_advect()
        want = np.array([(rho * a[j]).sum() for j in range(dim)])
        tol = 16.0 * eps * rho.sum()
        print(name, precision, step, gained, want, np.abs(gained - want), tol)
        assert np.all(np.abs(want) > 100.0 * tol)
        assert np.all(np.abs(gained - want) <= tol)
        assert not t.acc.any() and not t.real_view(t.accel_field).any()
