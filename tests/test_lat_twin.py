"""The numpy twin of a single-fluid BGK step with the lattice from tables (tests/_lat_twin.py), the yardstick of the D3Q15 /
D3Q27 GPU tests: its pieces against the reference's own sympy objects (tests/golden/arith_lat_*.npz,
tools/capture_lattices.py), the whole of it with the D3Q19 tables against the CPU oracle bit for bit, and a 2 x 2 x 2
decomposition exchanged through sailfish_amd.subdomain_connection against the uncut box.  No GPU."""
import os

import numpy as np
import pytest

from oracle.oracle import OracleSim
from sailfish_amd import sym
from sailfish_amd.geo import LBGeometry3D
from tests import _lat
from tests import _lat_twin as tw

# the bound of the same comparison for D3Q19 (tests/test_sc3_twin.py, tests/test_fe_twin.py): "a few ulp" -- the expressions
# have up to ~10 roundings of values below 2
ULPS = 8 * np.finfo(np.float64).eps


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_pieces_against_the_reference(name, golden_dir):
    grid = sym.lookup_grid(name)
    g = np.load(os.path.join(golden_dir, 'arith_lat_%s.npz' % name))
    R = np.float64
    rho, v, a = g['rho'].astype(R), [g['v'][:, d].astype(R) for d in range(3)], [g['accel'][:, d].astype(R) for d in range(3)]
    assert len(rho) >= 30 and rho.min() >= 0.8 and rho.max() <= 1.2 and np.linalg.norm(g['v'], axis=1).max() <= 0.1
    tau = float(g['tau'])
    assert tau == sym.relaxation_time(float(g['visc']))
    got = {
        'feq': tw.equilibrium(grid, rho, v, False, R).T,
        'feq_incompressible': tw.equilibrium(grid, rho, v, True, R).T,
        'guo': tw.guo_term(grid, rho, v, a, R(3.0 * (1.0 - 0.5 / tau)), R).T,
        'edm': tw.equilibrium(grid, rho, [c + b for c, b in zip(v, a)], False, R).T,
    }
    f = g['f'].T.astype(R)
    got['mom_rho'], mv = tw.macro(grid, f, False, R)
    got['mom_v'] = np.stack(mv, axis=1)
    got['mom_v_incompressible'] = np.stack(tw.macro(grid, f, True, R)[1], axis=1)
    worst = dict((k, float(np.max(np.abs(x - g[k])))) for k, x in got.items())
    print(name, ' '.join('%s %.2e' % kv for kv in sorted(worst.items())), '(bound %.2e)' % ULPS)
    for k, w in worst.items():
        assert got[k].shape == g[k].shape and w <= ULPS, (k, w)
    # the fixture is not degenerate: the terms it pins are there
    assert np.abs(g['guo']).max() > 1e-5 and np.abs(g['edm'] - g['feq']).max() > 1e-5
    assert np.abs(g['feq'] - g['feq_incompressible']).max() > 1e-4


ORACLE_BOXES = [('wall-box-guo', _lat.WALL_BOX), ('channel-halfway-edm', _lat.CHANNEL)]


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('box', [b for _, b in ORACLE_BOXES], ids=[n for n, _ in ORACLE_BOXES])
def test_twin_with_d3q19_tables_equals_the_oracle(box, pattern, precision):
    """20 and 21 steps: every wet slot of the arrays, bit for bit -- after 21 in-place steps they hold the populations
    un-streamed, in opposite slots.  Geometry, descriptor and node map come from the host layer for both."""
    sim, cfg = _lat.case('D3Q19', box, pattern=pattern, precision=precision)
    a = tw.TwinGroup(sim, LBGeometry3D, cfg)
    b = tw.TwinGroup(sim, LBGeometry3D, cfg, sim_of=OracleSim)
    kinds = a.merged('kind')
    wet = np.isin(kinds, tw.WET)
    walls = {'full': 4, 'half': 5}[box['walls']]
    assert (kinds == walls).any() and wet.any() and a.subs[0].desc.has_force == 1
    for steps in (20, 21):
        a.run(steps - a.subs[0].iteration)
        b.run(steps - b.subs[0].iteration)
        fa, fb = a.merged('dist'), b.merged('dist')
        assert np.all(np.isfinite(fa[:, wet]))
        assert np.array_equal(fa[:, wet], fb[:, wet]), (steps, int(np.count_nonzero(fa[:, wet] != fb[:, wet])))
        assert np.array_equal(a.merged('rho')[wet], b.merged('rho')[wet])
        for d in range(3):
            assert np.array_equal(a.merged('v%d' % d)[wet], b.merged('v%d' % d)[wet])


@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('name', _lat.LATTICES)
def test_halo_lists_carry_the_corner_links(name, pattern):
    """A 12 x 10 x 8 periodic box cut 2 x 2 x 2: every subdomain has 26 neighbour relations (seven distinct neighbours, some
    through several faces, edges and corners), exchanged through the index lists of subdomain_connection -- equal to the
    uncut box bit for bit, and the ghost-layer periodicity of the uncut box equals its in-sweep wrap."""
    sim, cfg = _lat.case(name, dict(size=(12, 10, 8), walls=None, force='guo'), pattern=pattern)
    steps = 9
    one = tw.TwinGroup(sim, LBGeometry3D, cfg).run(steps)
    many = tw.TwinGroup(sim, _lat.block_geometry([[6], [5], [4]]), cfg).run(steps)
    assert len(many.subs) == 8 and all(len(s.links) == 7 for s in many.subs)
    grid = sym.lookup_grid(name)
    corner = [i for i, e in enumerate(grid.basis) if all(e)]
    assert len(corner) == 8
    stride = tw.hipabi.dist_stride(many.subs[0].desc)
    sent = set(int(i) // stride for s in many.subs for l in s.links.values() for i in l.push_send)
    assert set(corner) <= sent
    want = one.merged('dist')
    assert np.all(np.isfinite(want))
    assert np.array_equal(want, many.merged('dist'))
    ghost = tw.TwinGroup(sim, LBGeometry3D, dict(cfg, hip_fused_periodic=False)).run(steps)
    assert np.array_equal(want, ghost.merged('dist'))


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_in_place_equals_two_copy_on_the_twin(name):
    sim, cfg = _lat.case(name, _lat.CHANNEL)
    ab = tw.TwinGroup(sim, LBGeometry3D, dict(cfg, access_pattern='AB')).run(8)
    aa = tw.TwinGroup(sim, LBGeometry3D, dict(cfg, access_pattern='AA')).run(8)
    assert np.array_equal(ab.merged('dist'), aa.merged('dist'))
