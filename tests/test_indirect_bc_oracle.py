"""Indirect addressing with boundary-condition nodes, on the CPU: for every configuration of the GPU matrix
(tests/test_gpu_indirect.py; the table is tests/_indirect_sims.py) the oracle group gives the same density, velocities and
populations on the fluid nodes with sparse and with dense distribution arrays, bit for bit.  The dense oracle is pinned to
the reference's expressions by tests/golden/; this pins the sparse one for inlets, outlets, outflow, slip and half-way
bounce-back nodes, which makes it the reference of the GPU runs.

And the one configuration that loses populations: half-way bounce-back walls, in-place pattern, an active-node map without
the layer behind the walls -- refused at set-up (SubdomainRunner._check_halfbb_targets)."""
import numpy as np
import pytest

from sailfish_amd import hipabi
from tests import _indirect_sims as S
from tests._oracle_group import OracleGroup

GEO = {2: 'EqualSubdomainsGeometry2D', 3: 'EqualSubdomainsGeometry3D'}


def _run(case, addressing, steps=None, **cfg_kw):
    og = OracleGroup(S.sim_class(case), case['dim'], GEO[case['dim']], dict(case['cfg'], node_addressing=addressing, **cfg_kw))
    with np.errstate(all='ignore'):
        og.run(case['steps'] if steps is None else steps, save_last=True)
    return og


def _fields(og, dim):
    return [og.merged('rho')] + [og.merged('v%d' % d) for d in range(dim)] + [og.merged('dist')]


def _assert_equal_on_fluid(ogd, ogi, dim, vmin):
    gshape = tuple(reversed(ogd.subs[0].runner._global_size))
    fluid = S.fluid_mask([s.runner for s in ogd.subs], gshape)
    assert np.array_equal(fluid, S.fluid_mask([s.runner for s in ogi.subs], gshape))
    assert fluid.sum() > 50
    fd, fi = _fields(ogd, dim), _fields(ogi, dim)
    for a, b in zip(fd[:-1], fi[:-1]):
        assert np.isfinite(a[fluid]).all()
        assert np.array_equal(a[fluid], b[fluid])
    assert np.array_equal(fd[-1][:, fluid], fi[-1][:, fluid])
    vmax = max(float(np.abs(c[fluid]).max()) for c in fi[1:-1])
    assert vmax > vmin, vmax                       # the flow moved


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_sparse_oracle_equals_dense_oracle(name):
    case = S.CASES[name]
    ogi = _run(case, 'indirect')
    for sub in ogi.subs:
        r = sub.runner
        assert sub.indirect and sub.desc.node_addressing == hipabi.SLF_ADDR_INDIRECT
        assert sub.desc.dist_stride < int(np.prod(r._physical_size))
        assert sub.desc.dist_stride >= r._subdomain.active_nodes + 1
    if not case['dense']:
        # the outlet behind the block: the dense run reads a wall node's storage where the sparse one has no slot to read --
        # the GPU run is compared with the sparse oracle, which has to stay finite on the fluid nodes
        gshape = tuple(reversed(ogi.subs[0].runner._global_size))
        fluid = S.fluid_mask([s.runner for s in ogi.subs], gshape)
        for a in _fields(ogi, case['dim'])[:-1]:
            assert np.isfinite(a[fluid]).all()
        assert np.isfinite(ogi.merged('dist')[:, fluid]).all()
        return
    _assert_equal_on_fluid(_run(case, 'direct'), ogi, case['dim'], case['vmin'])


@pytest.mark.parametrize('name', sorted(n for n in S.CASES if '_guard-' in n))
def test_outflow_nodes_behind_the_block_have_upstream_neighbours_without_a_slot(name):
    """What the `_guard` cases are for: the INVALID_NODE guards of the NTCopy / NTYuOutflow reads (slf_sweep.h) are taken."""
    case = S.CASES[name]
    og = _run(case, 'indirect', steps=0)
    sub = og.subs[0]
    r = sub.runner
    addr = sub.addr.reshape(sub.o.shape)
    vis = r._subdomain.visualization_map()
    outflow = getattr(S.nt, case['sim']['outlet']).id
    pos = np.argwhere(vis == outflow) + 1                          # real node -> ghost-including index
    assert len(pos) > 0
    # one / two nodes upstream = along the outlet's inward normal, in the case's frame (array axes are [z,] y, x)
    fa, fs, _ = S.frame_axes(case['dim'], case['sim'].get('frame'))
    up = np.zeros(3, dtype=np.int64)
    up[2 - fa] = -fs
    full = [np.array([p[0] if case['dim'] == 3 else 0, p[-2], p[-1]]) for p in pos]
    s1 = np.array([addr[tuple(p + up)] for p in full])
    s2 = np.array([addr[tuple(p + 2 * up)] for p in full])
    own = np.array([addr[tuple(p)] for p in full])
    assert np.all(own != hipabi.SLF_INVALID_NODE)
    missing = (s1 == hipabi.SLF_INVALID_NODE) | (s2 == hipabi.SLF_INVALID_NODE)
    assert missing.any() and not missing.all()


@pytest.mark.parametrize('name', sorted(S.SLOT_EDGES))
def test_slot_count_edges(name):
    case = S.CASES[name + '-20']
    sub = _run(case, 'indirect', steps=0).subs[0]
    n = sub.runner._subdomain.active_nodes
    assert S.SLOT_EDGES[name](n, int(sub.desc.dist_stride)), (n, int(sub.desc.dist_stride))


def test_the_standard_shapes_leave_inactive_nodes_and_pass_one_workgroup():
    for dim in (2, 3):
        case = S.CASES['regvel_zhrho-d%d-f32-bgk-AA-20' % dim]
        r = _run(case, 'indirect', steps=0).subs[0].runner
        mask = r._subdomain.active_node_mask
        assert r._subdomain.active_nodes > 256
        assert not mask[tuple(slice(1, -1) for _ in mask.shape)].all()      # inner nodes of the block own no slot
        assert case['cfg']['lat_nx'] < 64                                   # a row is shorter than a wave


# ---- half-way bounce-back walls in place: the map without the layer behind the walls is refused ---------------------------
def _halfbb_case(dim, pattern, halfbb_solid):
    sim = dict(dim=dim, wall='NTHalfBBWall', inlet='NTZouHeVelocity', outlet='NTEquilibriumDensity', halfbb_solid=halfbb_solid)
    return dict(sim=sim, dim=dim, cfg=S._cfg(dim, 'double', 'bgk', pattern), steps=20)


@pytest.mark.parametrize('dim', [2, 3])
def test_narrow_map_with_half_way_walls_in_place_is_refused(dim):
    """Before the check the run stayed finite and gave another flow: max |vx| on the fluid nodes after 20 steps 0.174 (2-D)
    and 0.182 (3-D) against 0.031 of the direct run -- the reflected populations of the even step were dropped."""
    case = _halfbb_case(dim, 'AA', True)
    with pytest.raises(ValueError, match=r'(\d+) links.*first at node \(.*layer behind') as info:
        _run(case, 'indirect', steps=0)
    assert int(info.value.args[0].split(' links')[0].split()[-1]) > 0
    for remedy in ('active-node map', 'full-way', 'two-copy'):
        assert remedy in str(info.value)
    _run(case, 'direct', steps=1)                         # dense arrays: nothing to refuse


def test_narrow_map_is_refused_in_single_precision_and_mrt_too():
    case = _halfbb_case(2, 'AA', True)
    case['cfg'].update(precision='single', model='mrt')
    with pytest.raises(ValueError, match='layer behind'):
        _run(case, 'indirect', steps=0)


@pytest.mark.parametrize('dim', [2, 3])
def test_wide_map_with_half_way_walls_in_place_equals_the_direct_run(dim):
    case = _halfbb_case(dim, 'AA', False)
    _assert_equal_on_fluid(_run(case, 'direct'), _run(case, 'indirect'), dim, 1e-3)
    narrow = _run(_halfbb_case(dim, 'AB', True), 'indirect', steps=0).subs[0].runner._subdomain.active_nodes
    wide = _run(case, 'indirect', steps=0).subs[0].runner._subdomain.active_nodes
    assert wide > narrow


@pytest.mark.parametrize('dim', [2, 3])
def test_narrow_map_in_the_two_copy_pattern_equals_the_direct_run(dim):
    """The two-copy step stores the reflected population into the node's own slot: nothing is lost."""
    case = _halfbb_case(dim, 'AB', True)
    _assert_equal_on_fluid(_run(case, 'direct'), _run(case, 'indirect'), dim, 1e-3)
