"""GPU parity: the hand-written gfx950 kernels (through the C ABI, via
backend_hip) against the CPU oracle on the same seeded inputs.

Tolerance (BASELINE.json north_star): 1e-6 relative on the macroscopic rho / u
fields (u relative to the velocity scale 0.05-0.1 of the cases).  Because the
kernels and the oracle follow the same IEEE operation order with FMA
contraction off, the populations are in practice bit-identical; that stronger
property is asserted for f32 fluid-only runs and reported otherwise.
"""
import numpy as np
import pytest

from sailfish_amd import hipabi, sym
from sailfish_amd.box import BoxSim, make_box_desc
from tests import _geometry as geo
from tests._oracle_box import OracleBox, synthetic_fields
from tests._pair import run_pair as _run_pair

pytestmark = pytest.mark.gpu

RTOL = 1e-6


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


BOX = [(sym.D2Q9, (70, 11)), (sym.D3Q19, (70, 6, 5))]


@pytest.mark.parametrize('grid,size', BOX)
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('fused', [0, 1])
@pytest.mark.parametrize('model', ['bgk', 'mrt'])
def test_periodic_box_f32(backend, grid, size, pattern, fused, model):
    r = _run_pair(backend, grid, size, 21, (True, True, True), model=model, precision='single',
                  access_pattern=pattern, visc=0.01, periodic_fused=[fused] * 3)
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    assert r['dist_exact'], r     # same IEEE operation order -> bit-identical populations


@pytest.mark.parametrize('grid,size', BOX)
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_periodic_box_f64(backend, grid, size, pattern):
    r = _run_pair(backend, grid, size, 12, (True, True, True), model='bgk', precision='double',
                  access_pattern=pattern, visc=1.0 / 6.0, periodic_fused=[0] * 3)
    assert r['rho_err'] < 1e-12 and r['v_err'] < 1e-12, r


@pytest.mark.parametrize('grid,size', BOX)
def test_body_force_and_incompressible(backend, grid, size):
    r = _run_pair(backend, grid, size, 10, (True, True, True), model='bgk', precision='single',
                  access_pattern='AA', visc=0.02, periodic_fused=[1] * 3, accel=[1e-5, -2e-5, 3e-5][:grid.dim],
                  incompressible=True)
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    r = _run_pair(backend, grid, size, 10, (True, True, True), model='mrt', precision='single',
                  access_pattern='AB', visc=0.02, periodic_fused=[0] * 3, accel=[1e-5, -2e-5, 3e-5][:grid.dim])
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    # moment-space forcing through the tuned fluid-only kernels (in-sweep wrap), both access patterns
    for pattern in ('AA', 'AB'):
        r = _run_pair(backend, grid, size, 10, (True, True, True), model='mrt', precision='single',
                      access_pattern=pattern, visc=0.02, periodic_fused=[1] * 3, accel=[1e-5, -2e-5, 3e-5][:grid.dim])
        assert r['rho_err'] < RTOL and r['v_err'] < RTOL and r['dist_exact'], r


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('model', ['bgk', 'mrt'])
def test_cavity_3d(backend, pattern, model):
    """regtest/ldc_3d-style cavity: full-BB walls + regularized-velocity lid."""
    r = _run_pair(backend, sym.D3Q19, (20, 14, 12), 40, (False, False, False), node_map_fn=geo.cavity_3d,
                  u_scale=0.05, init='rest', model=model, precision='single', access_pattern=pattern,
                  visc=0.03, fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS,
                  node_params=[0.05, 0.0, 0.0])
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
def test_cavity_2d(backend, pattern):
    r = _run_pair(backend, sym.D2Q9, (66, 40), 60, (False, False, False), node_map_fn=geo.cavity_2d,
                  u_scale=0.1, init='rest', model='bgk', precision='single', access_pattern=pattern,
                  visc=0.0254, fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS,
                  node_params=[0.1, 0.0])
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('fused', [0, 1])
def test_channel_2d_halfbb_force(backend, pattern, fused):
    grid = sym.D2Q9
    r = _run_pair(backend, grid, (40, 18), 50, (True, False, False),
                  node_map_fn=lambda d: geo.channel_2d_halfbb(grid, d), u_scale=0.01, init='rest',
                  model='bgk', precision='single', access_pattern=pattern, visc=0.05, fluid_only=False,
                  type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, periodic_fused=[fused, 0, 0], accel=[1e-5, 0.0],
                  use_link_tags=True)
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r


@pytest.mark.parametrize('model', ['bgk', 'mrt'])
def test_channel_2d_pressure(backend, model):
    r = _run_pair(backend, sym.D2Q9, (40, 18), 50, (False, False, False), node_map_fn=geo.channel_2d_pressure,
                  u_scale=0.01, init='rest', model=model, precision='single', access_pattern='AB', visc=0.05,
                  fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, node_params=[1.01, 0.99])
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r


def test_channel_3d_fullbb_force(backend):
    r = _run_pair(backend, sym.D3Q19, (24, 16, 10), 40, (True, False, True), node_map_fn=geo.channel_3d_fullbb,
                  u_scale=0.01, init='rest', model='bgk', precision='single', access_pattern='AA', visc=0.05,
                  fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, periodic_fused=[1, 0, 1],
                  accel=[1e-5, 0.0, 0.0])
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r


def test_region_launches_cover_domain(backend):
    """bulk/boundary split: sweeping z-planes in three launches == one launch."""
    grid, size = sym.D3Q19, (33, 9, 8)
    desc = make_box_desc(grid, size, precision='single', access_pattern='AB', visc=0.02, periodic_fused=[1, 1, 1])
    rho, v = synthetic_fields(size, 3)
    out = []
    for split in (False, True):
        s = BoxSim(backend, desc, periodic=(True, True, True))
        s.set_fields(rho, v)
        s.initial_conditions()
        for _ in range(4):
            if split:
                it = s.iteration
                s.iteration = it
                for reg in ((1, 10, 1, 2), (1, 10, 8, 9), (1, 10, 2, 8)):
                    s.backend.run_kernel(s.k_sweep[0][it & 1], reg, s.stream)
                s.iteration += 1
            else:
                s.step()
        out.append(s.real_view(s.get_dist()))
    assert np.array_equal(out[0], out[1])


def test_large_box_invariants(backend):
    """Size-independent properties at a bench-like size (256^3 would also do; kept at 128^3 for
    speed): mass and momentum conservation over 20 AA steps, AA == AB bitwise."""
    grid, n = sym.D3Q19, 128
    size = (n, n, n)
    rho, v = synthetic_fields(size, 3, dtype=np.float32)
    res = {}
    for pattern in ('AA', 'AB'):
        desc = make_box_desc(grid, size, precision='single', access_pattern=pattern, visc=0.01,
                             periodic_fused=[1, 1, 1])
        s = BoxSim(backend, desc, periodic=(True, True, True))
        s.set_fields(rho, v)
        s.initial_conditions()
        f0 = s.real_view(s.get_dist()).astype(np.float64)
        s.run(20, save_last=True)
        f1 = s.real_view(s.get_dist())
        res[pattern] = f1.copy()
        m0, m1 = f0.sum(), f1.astype(np.float64).sum()
        assert abs(m1 - m0) / m0 < 1e-6
        e = grid.basis_array
        for d in range(3):
            p0 = sum(e[i][d] * f0[i].sum() for i in range(grid.Q))
            p1 = sum(e[i][d] * f1[i].astype(np.float64).sum() for i in range(grid.Q))
            assert abs(p1 - p0) / m0 < 1e-6
        del s
    assert np.array_equal(res['AA'], res['AB'])


@pytest.mark.parametrize('variant', [1, 3, 9, 11])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('size', [(70, 6, 5), (130, 5, 4), (62, 4, 4), (191, 3, 3)])
def test_tuned_kernel_variants_bit_exact(backend, variant, pattern, size, monkeypatch):
    """The tuned north-star kernels (slf_fast.hip; non-temporal, vector, whole-row aligned
    streaming) must reproduce the oracle bit for bit, including rows that span several
    wavefronts and rows whose mirror lanes fall on wavefront boundaries."""
    monkeypatch.setenv('SLF_VARIANT', str(variant))
    for model in ('bgk', 'mrt'):
        r = _run_pair(backend, sym.D3Q19, size, 9, (True, True, True), model=model, precision='single',
                      access_pattern=pattern, visc=0.01, periodic_fused=[1, 1, 1])
        assert r['dist_exact'] and r['rho_err'] == 0.0 and r['v_err'] == 0.0, (variant, pattern, size, model, r)


@pytest.mark.parametrize('grid,size', [(sym.D2Q9, (40, 18)), (sym.D3Q19, (26, 12, 6))])
@pytest.mark.parametrize('t_in,t_out,model,pattern', [
    ('T_ZHVEL', 'T_ZHDENS', 'bgk', 'AB'), ('T_ZHVEL', 'T_ZHDENS', 'mrt', 'AA'),
    ('T_REGVEL', 'T_REGDENS', 'bgk', 'AA'), ('T_EQVEL', 'T_ZHDENS', 'bgk', 'AB'),
    ('T_ZHVEL', 'T_EQDENS', 'bgk', 'AA')])
def test_open_channel_inlet_outlet(backend, grid, size, t_in, t_out, model, pattern):
    """Zou-He velocity / density and regularized density nodes (reference boundary.mako:343-382, 487-506,
    811-835) in an open channel: velocity inlet, density outlet, full-BB walls."""
    dim = grid.dim
    params = [0.03, 0.0] + ([0.0] if dim == 3 else []) + [1.0]
    r = _run_pair(backend, grid, size, 60, (False, False, dim == 3),
                  node_map_fn=lambda d: geo.channel_inlet_outlet(d, getattr(geo, t_in), getattr(geo, t_out), dim),
                  u_scale=0.03, init='rest', model=model, precision='single', access_pattern=pattern, visc=0.05,
                  fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, node_params=params,
                  periodic_fused=[0, 0, 1 if dim == 3 else 0])
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    assert r['dist_exact'], r


@pytest.mark.parametrize('grid,size', [(sym.D2Q9, (40, 18)), (sym.D3Q19, (26, 12, 6))])
@pytest.mark.parametrize('t_out,model', [('T_COPY', 'bgk'), ('T_YU', 'bgk'), ('T_COPY', 'mrt')])
def test_open_channel_outflow_nodes(backend, grid, size, t_out, model):
    """NTCopy / NTYuOutflow outlets (reference boundary.mako:574-603, two-copy access pattern): the unknown
    populations of the outlet nodes come from the nodes one / two steps upstream."""
    dim = grid.dim
    params = [0.03, 0.0] + ([0.0] if dim == 3 else []) + [1.0]
    r = _run_pair(backend, grid, size, 80, (False, False, dim == 3),
                  node_map_fn=lambda d: geo.channel_inlet_outlet(d, geo.T_ZHVEL, getattr(geo, t_out), dim),
                  u_scale=0.03, init='rest', model=model, precision='single', access_pattern='AB', visc=0.05,
                  fluid_only=False, type_kind=geo.TYPE_KIND_OUTFLOW, nt_bits=geo.NT_BITS, node_params=params,
                  periodic_fused=[0, 0, 1 if dim == 3 else 0])
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    assert r['dist_exact'], r


@pytest.mark.parametrize('grid,size', [(sym.D2Q9, (40, 18)), (sym.D2Q9, (150, 12)), (sym.D3Q19, (26, 12, 6)),
                                       (sym.D3Q19, (70, 8, 5))])
@pytest.mark.parametrize('model,precision', [('bgk', 'single'), ('mrt', 'single'), ('bgk', 'double')])
def test_open_channel_do_nothing_outlet_in_place(backend, grid, size, model, precision):
    """NTDoNothing outlet under the in-place pattern (reference boundary.mako:862-876): the unknown populations of the
    outlet nodes keep their value -- stored into the node's own slot by the odd steps, into the ghost node behind it by
    the even ones.  Odd number of steps and even: both halves end a run."""
    dim = grid.dim
    params = [0.03, 0.0] + ([0.0] if dim == 3 else []) + [1.0]
    for steps in (61, 80):
        r = _run_pair(backend, grid, size, steps, (False, False, dim == 3),
                      node_map_fn=lambda d: geo.channel_inlet_outlet(d, geo.T_ZHVEL, geo.T_DONOTHING, dim),
                      u_scale=0.03, init='rest', model=model, precision=precision, access_pattern='AA', visc=0.05,
                      fluid_only=False, type_kind=geo.TYPE_KIND_INPLACE, nt_bits=geo.NT_BITS, node_params=params,
                      periodic_fused=[0, 0, 1 if dim == 3 else 0])
        assert r['rho_err'] < RTOL and r['v_err'] < RTOL, (steps, r)
        assert r['dist_exact'], (steps, r)


@pytest.mark.parametrize('grid,size', [(sym.D2Q9, (40, 18)), (sym.D3Q19, (26, 12, 6))])
def test_do_nothing_node_is_a_fluid_node_in_the_two_copy_pattern(backend, grid, size):
    """node_type.py:296-307: "in the AB memory layout, leaving the outflow nodes defined as NTFluid works just fine" --
    the kind is accepted there and does what a fluid node does: the same arrays as with T_FLUID in its place."""
    dim = grid.dim
    params = [0.03, 0.0] + ([0.0] if dim == 3 else []) + [1.0]
    kw = dict(u_scale=0.03, init='rest', model='bgk', precision='single', access_pattern='AB', visc=0.05,
              fluid_only=False, type_kind=geo.TYPE_KIND_INPLACE, nt_bits=geo.NT_BITS, node_params=params,
              periodic_fused=[0, 0, 1 if dim == 3 else 0])
    r = _run_pair(backend, grid, size, 40, (False, False, dim == 3),
                  node_map_fn=lambda d: geo.channel_inlet_outlet(d, geo.T_ZHVEL, geo.T_DONOTHING, dim), **kw)
    assert r['dist_exact'], r
    dists = []
    for t_out in (geo.T_DONOTHING, geo.T_FLUID):
        desc = make_box_desc(grid, size, **{k: v for k, v in kw.items() if k not in ('u_scale', 'init')})
        s = BoxSim(backend, desc, periodic=(False, False, dim == 3),
                   node_map=geo.channel_inlet_outlet(desc, geo.T_ZHVEL, t_out, dim))
        s.set_fields(np.ones(tuple(reversed(size))), [np.zeros(tuple(reversed(size))) for _ in range(dim)])
        s.initial_conditions()
        s.run(40, save_last=True)
        dists.append(s.real_view(s.get_dist()).copy())
    assert np.array_equal(dists[0], dists[1], equal_nan=True)


@pytest.mark.parametrize('grid,size', [(sym.D2Q9, (40, 18)), (sym.D2Q9, (130, 10)), (sym.D3Q19, (26, 12, 6))])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('model', ['bgk', 'mrt'])
def test_channel_between_slip_walls(backend, grid, size, pattern, model):
    """NTSlip (reference boundary.mako:837-855, sym.py:481-497): dry wall nodes that reflect specularly."""
    dim = grid.dim
    r = _run_pair(backend, grid, size, 50, (True, False, dim == 3),
                  node_map_fn=lambda d: geo.channel_slip_walls(d, dim), model=model, precision='single',
                  access_pattern=pattern, visc=0.05, fluid_only=False, type_kind=geo.TYPE_KIND_INPLACE,
                  nt_bits=geo.NT_BITS, periodic_fused=[1, 0, 1 if dim == 3 else 0])
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    assert r['dist_exact'], r


def test_do_nothing_nodes_in_place_need_direct_addressing(backend):
    from sailfish_amd.backend_hip import HIPFatalError
    desc = make_box_desc(sym.D2Q9, (16, 8), access_pattern="AA", fluid_only=False, type_kind=geo.TYPE_KIND_INPLACE,
                         nt_bits=geo.NT_BITS, visc=0.05, periodic_fused=[1, 1, 0])
    desc.node_addressing = hipabi.SLF_ADDR_INDIRECT
    desc.dist_stride = 16 * 8
    with pytest.raises(HIPFatalError, match='NTDoNothing'):
        backend.build(desc)


def test_outflow_nodes_need_the_two_copy_pattern(backend):
    from sailfish_amd.backend_hip import HIPFatalError
    desc = make_box_desc(sym.D2Q9, (16, 8), access_pattern="AA", fluid_only=False, type_kind=geo.TYPE_KIND_OUTFLOW,
                         nt_bits=geo.NT_BITS, visc=0.05)
    with pytest.raises(HIPFatalError, match='two-copy'):
        backend.build(desc)


@pytest.mark.parametrize('nx', [150, 330])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('case', ['periodic_f32', 'periodic_f64_mrt', 'ghost_pbc_x', 'cavity', 'pipe_like'])
def test_odd_row_lengths(backend, nx, pattern, case):
    """Rows of 3 and 6 waves whose last wave is partly idle (128 + 22 and 256 + 74 nodes): around the periodic seam
    and into the ghost columns.  Bit-identical to the oracle.  (Rows cut into x-segments -- what leaves a segment is
    stored by its edge lane -- are what rows longer than 1024 nodes run: test_rows_longer_than_a_workgroup.)"""
    size = (nx, 6, 5)
    kw = dict(u_scale=0.05, access_pattern=pattern, visc=0.03)
    if case == 'periodic_f32':
        r = _run_pair(backend, sym.D3Q19, size, 13, (True, True, True), model='bgk', precision='single',
                      periodic_fused=[1, 1, 1], **kw)
    elif case == 'periodic_f64_mrt':
        r = _run_pair(backend, sym.D3Q19, size, 13, (True, True, True), model='mrt', precision='double',
                      periodic_fused=[1, 1, 1], **kw)
    elif case == 'ghost_pbc_x':      # x periodic through the ghost-layer kernels: rows are not wrapped in-sweep
        r = _run_pair(backend, sym.D3Q19, size, 13, (True, True, True), model='bgk', precision='single',
                      periodic_fused=[0, 1, 1], **kw)
    elif case == 'cavity':
        r = _run_pair(backend, sym.D3Q19, size, 13, (False, False, False), node_map_fn=geo.cavity_3d, init='rest',
                      model='bgk', precision='single', fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS,
                      node_params=[0.05, 0.0, 0.0], **kw)
    else:                            # unused nodes in the middle of rows, x wrapped in-sweep
        def holes(desc):
            m = geo.empty_map(desc)
            m[2:4, 2:5, 60:140] = geo.encode(geo.T_FULLBB)
            m[3, 3, 61:139] = geo.encode(geo.T_UNUSED)
            return m
        r = _run_pair(backend, sym.D3Q19, size, 13, (True, True, True), node_map_fn=holes, init='rest', model='bgk',
                      precision='single', fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS,
                      periodic_fused=[1, 1, 1], accel=[1e-5, 0.0, 0.0], **kw)
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    assert r['dist_exact'], r


FULL_WAVE_NX = [64, 128, 256, 512, 1024]
LONG_ROW_NX = [576, 700, 1000]      # two nodes per thread (slf_fast.hip NSEG = 2), second segment full / partial


@pytest.mark.parametrize('nx', FULL_WAVE_NX + LONG_ROW_NX)
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('model', ['bgk', 'mrt'])
def test_full_wave_rows_headline_kernels(backend, nx, pattern, model):
    """The headline shape: rows that fill their wavefronts exactly (nx = 64 k; 512 is the benchmark row).
    x == nx is lane 63 of the last wave, the LDS slot of the wave 'after' the last one is read but never
    written, the vec-2 even AA kernel has no tail -- none of which the idle-lane sizes exercise.  Fluid-only
    periodic box with in-sweep wrap = fast_row_kernel / fast_even_kernel (slf_fast.hip), f32, bit-exact
    against the oracle (reference propagation.mako:180-288; its warp-edge KATs: 2d_propagation.py:178-221)."""
    r = _run_pair(backend, sym.D3Q19, (nx, 4, 3), 7, (True, True, True), model=model, precision='single',
                  access_pattern=pattern, visc=0.01, periodic_fused=[1, 1, 1])
    assert r['dist_exact'] and r['rho_err'] == 0.0 and r['v_err'] == 0.0, (nx, pattern, model, r)


@pytest.mark.parametrize('nx', FULL_WAVE_NX)
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('case', ['generic_row_f32', 'generic_row_f64_mrt', 'ghost_pbc_x', 'cavity', 'holes'])
def test_full_wave_rows_row_kernels(backend, nx, pattern, case, monkeypatch):
    """Same row shapes through row_kernel / even_kernel (slf_row.hip): the generic fluid-only instantiation
    (SLF_VARIANT bit 256 routes around slf_fast.hip), f64 MRT, rows that are not wrapped in-sweep (ghost
    columns written by the edge lanes) and the GENERAL node-map instantiations (walls + lid; excluded nodes
    in the middle of rows)."""
    size = (nx, 4, 3)
    kw = dict(u_scale=0.05, access_pattern=pattern, visc=0.03)
    if case == 'generic_row_f32':
        monkeypatch.setenv('SLF_VARIANT', str(11 + 256))
        r = _run_pair(backend, sym.D3Q19, size, 7, (True, True, True), model='bgk', precision='single',
                      periodic_fused=[1, 1, 1], **kw)
    elif case == 'generic_row_f64_mrt':
        r = _run_pair(backend, sym.D3Q19, size, 7, (True, True, True), model='mrt', precision='double',
                      periodic_fused=[1, 1, 1], **kw)
    elif case == 'ghost_pbc_x':
        r = _run_pair(backend, sym.D3Q19, size, 7, (True, True, True), model='bgk', precision='single',
                      periodic_fused=[0, 1, 1], **kw)
    elif case == 'cavity':
        r = _run_pair(backend, sym.D3Q19, (nx, 5, 4), 7, (False, False, False), node_map_fn=geo.cavity_3d,
                      init='rest', model='bgk', precision='single', fluid_only=False, type_kind=geo.TYPE_KIND,
                      nt_bits=geo.NT_BITS, node_params=[0.05, 0.0, 0.0], **kw)
    else:
        def holes(desc):
            m = geo.empty_map(desc)
            m[1:4, 1:4, 30:nx - 10] = geo.encode(geo.T_FULLBB)
            m[2, 2, 31:nx - 11] = geo.encode(geo.T_UNUSED)      # enclosed by walls in all 19 directions
            return m
        r = _run_pair(backend, sym.D3Q19, (nx, 5, 5), 7, (True, True, True), node_map_fn=holes, init='rest',
                      model='mrt', precision='single', fluid_only=False, type_kind=geo.TYPE_KIND,
                      nt_bits=geo.NT_BITS, periodic_fused=[1, 1, 1], accel=[1e-5, 0.0, 0.0], **kw)
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    assert r['dist_exact'], r


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('model', ['bgk', 'mrt'])
@pytest.mark.parametrize('force', [False, True])
@pytest.mark.parametrize('nx', [70, 512])
def test_node_map_kernels_per_boundary_condition_level(backend, nx, force, model, pattern, monkeypatch):
    """The f32 whole-row node-map kernels exist once per Geometry::bc_level (slf_kernels.h): 0 = the type table holds
    nothing beyond fluid / ghost / unused / full-way bounce-back (52 VGPRs), 1 = boundary-condition nodes, 2 = also
    the outflow nodes of the two-copy pattern.  Same geometry (walls, holes, a body force or not) through level 0
    (plain table), level 1 (full table) and the level 2 instantiation (forced): every one bit-identical to the oracle."""
    from sailfish_amd import hipabi as h
    plain = (h.SLF_NK_FLUID, h.SLF_NK_GHOST, h.SLF_NK_FULL_BB, h.SLF_NK_UNUSED)

    def holes(desc):
        m = geo.empty_map(desc)
        m[1:4, 1:4, 30:nx - 10] = geo.encode(geo.T_FULLBB)
        m[2, 2, 31:nx - 11] = geo.encode(geo.T_UNUSED)
        m[1:6, 4, 5:9] = geo.encode(geo.T_FULLBB)
        return m
    for table, forced in (([k if k in plain else h.SLF_NK_UNUSED for k in geo.TYPE_KIND], None), (geo.TYPE_KIND, None),
                          (geo.TYPE_KIND, '2')):
        if forced:
            monkeypatch.setenv('SLF_BC_LEVEL', forced)
        r = _run_pair(backend, sym.D3Q19, (nx, 5, 5), 7, (True, True, True), node_map_fn=holes, init='rest', model=model,
                      precision='single', fluid_only=False, type_kind=table, nt_bits=geo.NT_BITS,
                      periodic_fused=[1, 1, 1], accel=[1e-5, -2e-5, 0.0] if force else None, u_scale=0.05,
                      access_pattern=pattern, visc=0.03)
        assert r['rho_err'] < RTOL and r['v_err'] < RTOL and r['dist_exact'], (table is geo.TYPE_KIND, forced, r)


@pytest.mark.parametrize('nx', [1088, 1536, 2100])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('case', ['periodic_f32', 'periodic_f32_mrt', 'periodic_f64', 'ghost_pbc_x', 'cavity', 'holes'])
def test_rows_longer_than_a_workgroup(backend, nx, pattern, case):
    """nx > 1024: no whole-row workgroup; the x-streaming steps cut the row into equal segments of at most 8 waves
    (slf_row.hip: row_block_x -- 3 x 384, 3 x 512, 5 x 448 nodes, the last one partly idle), the even AA step runs per
    node (fast_even_kernel / even_kernel with gridDim.x > 1).  Bit-identical to the oracle across the segment
    boundaries, around the periodic seam and into the ghost columns."""
    size = (nx, 4, 3)
    kw = dict(u_scale=0.05, access_pattern=pattern, visc=0.03)
    if case in ('periodic_f32', 'periodic_f32_mrt', 'periodic_f64'):
        r = _run_pair(backend, sym.D3Q19, size, 7, (True, True, True), model='mrt' if case.endswith('mrt') else 'bgk',
                      precision='double' if case.endswith('f64') else 'single', periodic_fused=[1, 1, 1], **kw)
    elif case == 'ghost_pbc_x':
        r = _run_pair(backend, sym.D3Q19, size, 7, (True, True, True), model='bgk', precision='single',
                      periodic_fused=[0, 1, 1], **kw)
    elif case == 'cavity':
        r = _run_pair(backend, sym.D3Q19, (nx, 5, 4), 7, (False, False, False), node_map_fn=geo.cavity_3d,
                      init='rest', model='bgk', precision='single', fluid_only=False, type_kind=geo.TYPE_KIND,
                      nt_bits=geo.NT_BITS, node_params=[0.05, 0.0, 0.0], **kw)
    else:
        def holes(desc):
            m = geo.empty_map(desc)
            m[1:4, 1:4, 300:nx - 200] = geo.encode(geo.T_FULLBB)
            m[2, 2, 301:nx - 201] = geo.encode(geo.T_UNUSED)
            return m
        r = _run_pair(backend, sym.D3Q19, (nx, 5, 5), 7, (True, True, True), node_map_fn=holes, init='rest',
                      model='mrt', precision='single', fluid_only=False, type_kind=geo.TYPE_KIND,
                      nt_bits=geo.NT_BITS, periodic_fused=[1, 1, 1], accel=[1e-5, 0.0, 0.0], **kw)
    assert r['rho_err'] < RTOL and r['v_err'] < RTOL, r
    assert r['dist_exact'], r


@pytest.mark.parametrize('pattern', ['AA', 'AB'])
def test_placed_distribution_arrays(backend, pattern, monkeypatch):
    """Distribution arrays as placed buffers (sailfish_amd/placement.py: one virtual range backed by separately
    created physical chunks with spacers in between while they are created): same results as a plain allocation,
    bit for bit -- including host copies that cross chunk boundaries -- and everything is given back."""
    from sailfish_amd import placement
    monkeypatch.setattr(placement, 'MIN_BYTES', 0)
    monkeypatch.setenv('SLF_PLACEMENT_SPAN_GIB', '1')
    size = (128, 24, 20)
    r = _run_pair(backend, sym.D3Q19, size, 9, (True, True, True), model='bgk', precision='single',
                  access_pattern=pattern, visc=0.01, periodic_fused=[1, 1, 1])
    assert r['dist_exact'] and r['rho_err'] == 0.0 and r['v_err'] == 0.0, r
    desc = make_box_desc(sym.D3Q19, size, access_pattern=pattern, periodic_fused=[1, 1, 1])
    used = backend.allocated_bytes()
    s = BoxSim(backend, desc, periodic=(True, True, True))
    assert len(s.placed) == (1 if pattern == 'AA' else 2) and s.placement_info['parts'] == placement.PARTS
    assert all(h is not None for pb in s.placed for h in pb.mapped)
    addrs = [pb.addr for pb in s.placed]
    s.release()
    assert not any(a in backend._placed for a in addrs) and backend.allocated_bytes() == used


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('model', ['bgk', 'mrt'])
@pytest.mark.parametrize('nx', [100, 512, 1100])
def test_row_classes_split_launch(backend, nx, pattern, model, monkeypatch):
    """slf_module_classify_rows: plain-fluid 64-node segments skip the node map, rows with boundary-condition nodes
    run the module's full instantiation from a row list and all other rows the level-0 one.  A cavity with lid (rows
    with and without boundary-condition nodes, mixed and all-fluid segments), swept in three regions: same results
    as the oracle bit for bit, and as the unsplit launch (SLF_ROW_CLASSES=0)."""
    size = (nx, 9, 8)
    kw = dict(model=model, precision='single', access_pattern=pattern, visc=0.03, fluid_only=False,
              type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, node_params=[0.05, 0.0, 0.0])
    desc = make_box_desc(sym.D3Q19, size, **kw)
    nmap = geo.cavity_3d(desc)
    nmap[3:6, 3:6, 200:260 if nx > 300 else 40:60] = geo.encode(geo.T_FULLBB)     # a block inside: class-1 segments
    shape = tuple(reversed(size))
    rho, v = np.ones(shape), [np.zeros(shape) for _ in range(3)]
    res = {}
    for split in ('1', '0'):
        monkeypatch.setenv('SLF_ROW_CLASSES', split)
        g = BoxSim(backend, make_box_desc(sym.D3Q19, size, **kw), periodic=(False, False, False), node_map=nmap)
        if split == '1':
            rc = g.row_classes
            assert rc['rows'] == 9 * 8 and 0 < rc['bc_rows'] < rc['rows'], rc
            assert 0 < rc['fluid_segments'] < rc['segments'] or nx <= 128, rc
        else:
            assert g.row_classes is None
        g.set_fields(rho, v)
        g.initial_conditions()
        for i in range(9):
            k = g.k_sweep[int(i == 8)][0 if g.aa else (g.iteration & 1)]
            for reg in ((1, 10, 1, 3), (1, 4, 3, 9), (4, 10, 3, 9)):     # regions: the row list is filtered per launch
                backend.run_kernel(k, reg, g.stream)
            g.iteration += 1
            backend.set_iteration(g.iteration)
        res[split] = (g.real_view(g.get_dist()).copy(), [c.copy() for c in g.fetch_fields()[1]])
        g.release()
    o = OracleBox(make_box_desc(sym.D3Q19, size, **kw), periodic=(False, False, False), node_map=nmap)
    o.set_fields(rho, v)
    o.initial_conditions()
    o.run(9, save_last=True)
    ref = o.real_view(o.current_dist())
    fin = np.isfinite(ref)
    for split in ('1', '0'):
        assert np.array_equal(res[split][0][fin], ref[fin]), split
    wet = np.isfinite(o.real_view(o.rho))
    for d in range(3):
        assert np.array_equal(o.real_view(res['1'][1][d])[wet], o.real_view(o.v[d])[wet])


@pytest.mark.parametrize('grid,size', BOX)
@pytest.mark.parametrize('case', ['periodic', 'force', 'channel'])
def test_minimize_roundoff_formulation(backend, grid, size, case):
    """--minimize_roundoff (slf_module_desc::incompressible = SLF_DENSITY_ROUNDOFF; arrays hold f_i - w_i): the kernels
    against the oracle bit for bit, the in-place pattern against the two-copy one bit for bit (the reference's
    tests/gpu/access_pattern.sh invariant), and against the standard formulation: same flow, density field smaller by
    exactly one."""
    from sailfish_amd import hipabi
    kw = dict(model='bgk', precision='single', visc=0.02, periodic_fused=[1, 1, 1])
    nmap = None
    if case == 'force':
        kw['accel'] = [1e-5, -2e-5, 0.0][:grid.dim]
    elif case == 'channel':
        kw.update(fluid_only=False, type_kind=geo.TYPE_KIND[:3], nt_bits=geo.NT_BITS, accel=[1e-5, 0.0, 0.0][:grid.dim])

        def nmap(desc):
            m = geo.empty_map(desc)
            m[..., 1, 1:desc.lat_nx - 1] = geo.encode(geo.T_FULLBB)
            m[..., desc.lat_ny - 2, 1:desc.lat_nx - 1] = geo.encode(geo.T_FULLBB)
            if desc.lat_nz > 1:
                m[0], m[-1] = geo.encode(geo.T_GHOST), geo.encode(geo.T_GHOST)
            return m
    res = {}
    for pattern in ('AB', 'AA'):
        r = _run_pair(backend, grid, size, 12, (True, True, True), node_map_fn=nmap, access_pattern=pattern,
                      incompressible=hipabi.SLF_DENSITY_ROUNDOFF, **kw)
        assert r['dist_exact'] and r['rho_err'] < RTOL and r['v_err'] < RTOL, (pattern, r)
    # AB == AA, and the standard formulation: identical physics
    out = {}
    for tag, dens, pattern in (('ro_ab', hipabi.SLF_DENSITY_ROUNDOFF, 'AB'), ('ro_aa', hipabi.SLF_DENSITY_ROUNDOFF, 'AA'),
                               ('std', 0, 'AA')):
        desc = make_box_desc(grid, size, access_pattern=pattern, incompressible=dens, **kw)
        s = BoxSim(backend, desc, periodic=(True, True, True), node_map=nmap(desc) if nmap else None)
        rho, v = synthetic_fields(size, grid.dim)
        s.set_fields(rho, v)
        s.initial_conditions()
        s.run(12, save_last=True)
        f = s.real_view(s.get_dist()).copy()
        frho, fv = s.fetch_fields()
        out[tag] = (f, s.real_view(frho).copy(), [s.real_view(c).copy() for c in fv])
        s.release()
    assert np.array_equal(out['ro_ab'][0], out['ro_aa'][0], equal_nan=True)
    wet = np.isfinite(out['std'][1]) & (out['std'][1] != 0)
    if nmap is not None:          # wall nodes keep whatever the host wrote into the density field: fluid nodes only
        desc = make_box_desc(grid, size, access_pattern='AA', **kw)
        fluid = (nmap(desc) & ((1 << geo.NT_BITS[0]) - 1)) == geo.T_FLUID
        d = desc
        fluid = fluid[1:d.lat_nz - 1, 1:d.lat_ny - 1, 1:d.lat_nx - 1] if grid.dim == 3 else fluid[0, 1:d.lat_ny - 1, 1:d.lat_nx - 1]
        wet = wet & fluid
    # (the standard formulation is the one that rounds more -- that is what the option is for: 12 steps in f32 leave the
    # two a few 1e-7 apart; in f64 they agree to 1e-15, tests/test_gpu_golden.py pins both to the reference's expressions)
    assert np.max(np.abs((out['ro_aa'][1][wet] + 1.0) - out['std'][1][wet])) < 5e-6
    for d in range(grid.dim):
        assert np.max(np.abs(out['ro_aa'][2][d][wet] - out['std'][2][d][wet])) < 1e-6
