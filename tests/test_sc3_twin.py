"""The numpy twin of the N-component Shan-Chen mixture (tests/_scn_twin.py), the yardstick of the ternary GPU tests:
its pieces against the reference's own sympy objects (tests/golden/arith_sc3_*.npz, tools/capture_sc3.py), the whole of it
with N = 2 against the CPU oracle's binary model bit for bit, and mass conservation with N = 3.  No GPU."""
import os

import numpy as np
import pytest

from oracle import oracle
from sailfish_amd import hipabi, sym
from tests import _sc3
from tests import _scn_twin as tw

GRIDS = [sym.D2Q9, sym.D3Q19]
ULPS = 8 * np.finfo(np.float64).eps      # "a few ulp": the expressions have up to ~10 roundings of values below 2


def _golden(golden_dir, grid):
    return np.load(os.path.join(golden_dir, 'arith_sc3_%s.npz' % grid.__name__))


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: g.__name__)
def test_couplings_of_the_fixture_are_the_products(grid, golden_dir):
    """constants() of the reference for six distinct couplings: symmetric pairs; its force couplings in iteration order are
    (0, 0) .. (2, 2) row by row -- the order the kernels and the twin add them in -- and the product's class agrees."""
    g = _golden(golden_dir, grid)
    consts = dict(zip([str(n) for n in g['coupling_names']], g['coupling_values']))
    assert len(set(g['G'])) == 6 and np.all(g['G'] != 0)
    for a, b in (('G12', 'G21'), ('G13', 'G31'), ('G23', 'G32')):
        assert consts[a] == consts[b]
    assert g['force_couplings'].tolist() == [[k, j] for k in range(3) for j in range(3)]
    assert [str(n) for n in g['force_coupling_names']] == ['G%d%d' % (k + 1, j + 1) for k in range(3) for j in range(3)]

    class Cfg(object):
        grid_name = grid.__name__
    cfg = Cfg()
    cfg.grid = grid.__name__
    for name, val in zip(('G11', 'G12', 'G13', 'G22', 'G23', 'G33'), g['G']):
        setattr(cfg, name, float(val))
    from sailfish_amd.lb_ternary import LBTernaryFluidShanChen
    sim = LBTernaryFluidShanChen(cfg)
    mine = sim.constants()
    assert dict((k, mine[k]) for k in consts) == consts
    assert list(sim._force_couplings.items()) == [((int(k), int(j)), str(n)) for (k, j), n in
                                                  zip(g['force_couplings'], g['force_coupling_names'])]
    assert _sc3.couplings(_sc3.PARAMS) == [[consts['G%d%d' % (k + 1, j + 1)] for j in range(3)] for k in range(3)]
    assert np.array_equal(g['tau'], [sym.relaxation_time(_sc3.PARAMS['visc']), _sc3.PARAMS['tau_phi'], _sc3.PARAMS['tau_theta']])


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: g.__name__)
def test_equilibria_and_guo_terms_against_the_reference(grid, golden_dir):
    g = _golden(golden_dir, grid)
    R = np.float64
    worst = dict(feq=0.0, guo=0.0)
    for k in range(len(g['dens'])):
        v = [R(c) for c in g['v'][k]]
        for num in range(3):
            rho = R(g['dens'][k, num])
            fe = tw.feq(grid, rho, v, R)
            worst['feq'] = max(worst['feq'], float(np.max(np.abs(fe - g['feq'][k, num]))))
            a = [R(c) for c in g['accel'][k, num]]
            gt = tw.guo_term(grid, rho, [np.asarray(c) for c in v], [np.asarray(c) for c in a], g['tau'][num], R)
            worst['guo'] = max(worst['guo'], float(np.max(np.abs(gt - g['guo'][k, num]))))
    print('%s: |feq - reference| %.2e, |guo - reference| %.2e (bound %.2e)' % (grid.__name__, worst['feq'], worst['guo'], ULPS))
    assert worst['feq'] <= ULPS and worst['guo'] <= ULPS


@pytest.mark.parametrize('exp', ['libm', 'numpy'])
def test_pseudopotentials_against_the_reference(golden_dir, exp):
    g = _golden(golden_dir, sym.D2Q9)
    assert np.array_equal(tw.psi(g['psi_rho'], 'linear', np.float64, exp), g['psi_linear'])
    got = tw.psi(g['psi_rho'], 'classic', np.float64, exp)
    worst = float(np.max(np.abs(got - g['psi_classic'])))
    print('classic potential (%s exp): %.2e' % (exp, worst))
    assert worst <= 2 * np.finfo(np.float64).eps       # exp within an ulp of values below 1, one subtraction


# ---- N = 2: the twin equals the CPU oracle's binary model ---------------------------------------------------------------

def _oracle_binary(grid, size, dtype, steps, tau, G, potential, accel, wall, fields):
    """`steps` two-copy steps of the oracle's binary Shan-Chen model on a box periodic along every axis (wrapped inside the
    sweep); returns the populations and fields of the real nodes."""
    dim = grid.dim
    lat = [n + 2 for n in size] + [1] * (3 - dim)
    kw = dict(lattice=grid.slf_id, model=hipabi.SLF_BGK, precision=np.dtype(dtype).itemsize, access_pattern=hipabi.SLF_AB,
              lat_nx=lat[0], lat_ny=lat[1], lat_nz=lat[2], arr_nx=lat[0], arr_ny=lat[1], arr_nz=lat[2],
              periodic_fused=[1] * dim + [0] * (3 - dim), periodic_local=[1] * dim + [0] * (3 - dim),
              tau=tau[0], visc=(2.0 * tau[0] - 1.0) / 6.0, tau_phi=tau[1], simtype=hipabi.SLF_SIM_SHAN_CHEN_BINARY,
              sc_G=[G[0][0], G[0][1], G[1][0], G[1][1]], sc_potential=0 if potential == 'linear' else 1,
              accel=list(accel[0]) + [0.0] * (3 - dim), accel1=list(accel[1]) + [0.0] * (3 - dim),
              has_force=int(any(c != 0.0 for c in accel[0])), fluid_only=int(wall is None))
    if wall is not None:
        kw.update(nt_type_mask=3, nt_misc_shift=2, type_kind=[hipabi.SLF_NK_FLUID, hipabi.SLF_NK_FULL_BB, hipabi.SLF_NK_GHOST])
    desc = hipabi.make_desc(**kw)
    o = oracle.OracleSim(desc)
    real = tuple(slice(1, n + 1) for n in reversed(size))
    if dim == 2:
        real = (slice(0, 1),) + real
    nmap = None
    if wall is not None:
        nmap = np.full(o.shape, 2, dtype=np.uint32)
        nmap[real] = np.where(wall, 1, 0).reshape(nmap[real].shape)
    rho, phi = o.new_field(1.0), o.new_field(1.0)
    rho[real] = fields[0].reshape(rho[real].shape)
    phi[real] = fields[1].reshape(phi[real].shape)
    v = [o.new_field(0.0) for _ in range(3)]
    d = [[o.new_dist(), o.new_dist()], [o.new_dist(), o.new_dist()]]      # [lattice][copy]
    for c in (0, 1):
        o.sc_init(d[0][c], d[1][c], rho, phi, v[0], v[1], v[2])
    for it in range(steps):
        i, j = it & 1, 1 - (it & 1)
        o.sc_macro(0, nmap, d[0][i], d[1][i], rho, phi, v[0], v[1], v[2])
        o.sc_step(0, 0, nmap, d[0][i], d[0][j], rho, phi, v[0], v[1], v[2])
        o.sc_step(1, 0, nmap, d[1][i], d[1][j], rho, phi, v[0], v[1], v[2])
    cur = steps & 1
    shape = tuple(reversed(size))
    pops = [d[k][cur][(slice(None),) + real].reshape((grid.Q,) + shape) for k in (0, 1)]
    return pops, [a[real].reshape(shape) for a in (rho, phi)], [a[real].reshape(shape) for a in v[:dim]]


def _binary_case(grid, dtype, potential, walls=False, edm=False):
    dim = grid.dim
    size = (12, 14) if dim == 2 else (7, 14, 6)
    shape = tuple(reversed(size))
    tau = [sym.relaxation_time(0.09), 0.87]
    G = [[-0.31, 0.92], [0.92, -0.27]]
    accel = [[0.0] * dim, [1e-4, -2e-4, 3e-4][:dim]]
    rng = np.random.RandomState(5)
    fields = [(1.0 + 0.02 * rng.rand(*shape)).astype(dtype), (0.7 + 0.02 * rng.rand(*shape)).astype(dtype)]
    wall = None
    if walls:
        idx = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
        wall = _sc3.solid(dim, list(reversed(idx)), size[1])
    return size, tau, G, accel, fields, wall


@pytest.mark.parametrize('walls', [False, True], ids=['periodic', 'walls'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: g.__name__)
def test_binary_twin_equals_the_oracle_bit_for_bit(grid, dtype, walls):
    """20 steps, linear potential, G11, G12, G22 all non-zero, tau_phi != tau, a body force on lattice 1: populations and
    fields bit-identical.  This carries the oracle's pinned arithmetic over to the twin.  (The oracle is driven through
    oracle.OracleSim: the CPU test backend serves single-fluid kernel names only.)"""
    steps = 20
    size, tau, G, accel, fields, wall = _binary_case(grid, dtype, 'linear', walls)
    pops, dens, v = _oracle_binary(grid, size, dtype, steps, tau, G, 'linear', accel, wall, fields)
    t = tw.ScTwin(grid, tuple(reversed(size)), dtype, tau, G, 'linear', accel, wall=wall)
    t.set_fields(fields, [np.zeros(t.shape)] * grid.dim)
    for _ in range(steps - 1):
        t.step()
    t.step()
    for k in (0, 1):
        assert t.f[k].dtype == dtype
        assert np.array_equal(t.f[k], pops[k]), 'lattice %d' % k
        assert np.array_equal(t.field[k], dens[k]), 'field %d' % k      # the fields of the last step's pass in front
    for d in range(grid.dim):
        assert np.array_equal(t.v[d], v[d])
    assert not np.array_equal(t.f[0], tw.feq(grid, fields[0], [np.zeros(t.shape, dtype)] * grid.dim, dtype))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: g.__name__)
def test_binary_twin_equals_the_oracle_classic_potential_and_edm(grid, dtype):
    """The classic potential: the twin evaluates exp as the oracle does -- the C library's double-precision exp, the result
    rounded to the working format (_scn_twin.psi(exp='libm')) -- so the bits are demanded here too; 10 steps."""
    steps = 10
    size, tau, G, accel, fields, wall = _binary_case(grid, dtype, 'classic')
    G = [[-1.9, 1.4], [1.4, -2.3]]
    pops, dens, v = _oracle_binary(grid, size, dtype, steps, tau, G, 'classic', accel, wall, fields)
    t = tw.ScTwin(grid, tuple(reversed(size)), dtype, tau, G, 'classic', accel, wall=wall, exp='libm')
    t.set_fields(fields, [np.zeros(t.shape)] * grid.dim)
    for _ in range(steps):
        t.step()
    for k in (0, 1):
        assert np.array_equal(t.f[k], pops[k]) and np.array_equal(t.field[k], dens[k])


# ---- N = 3 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_ternary_twin_conserves_each_component(dtype):
    """Periodic 32 x 16 D2Q9 box, 200 steps.  Streaming moves values unchanged; a collision changes a node's density by the
    rounding of its Q updates (relaxation and forcing: four roundings each) and of the Q-term sum: at most 5 Q half-ulps of
    values below the node's density (< 1.1), in every step.  The bound lets that add up over every node and step."""
    size, steps, Q = (32, 16), 200, 9
    t = _sc3.make_twin(2, size, dtype, G11=-0.1, G12=0.3, G13=0.25, G22=-0.09, G23=0.35, G33=-0.06)
    m0 = [float(f.astype(np.float64).sum()) for f in t.f]
    for _ in range(steps):
        t.step()
    m1 = [float(f.astype(np.float64).sum()) for f in t.f]
    n, eps = int(np.prod(size)), float(np.finfo(dtype).eps)
    bound = n * steps * 5 * Q * 0.5 * eps * 1.1
    drift = [abs(a - b) for a, b in zip(m0, m1)]
    print('drift of rho, phi, theta: %.3e %.3e %.3e (bound %.3e)' % (drift[0], drift[1], drift[2], bound))
    assert all(np.all(np.isfinite(f)) for f in t.f)
    assert max(drift) <= bound
