"""D3Q15 and D3Q27 on the host, no GPU: the tables of sailfish_amd/sym.py and of csrc/slf_lattice.h against the reference's
(tests/golden/lattices_q15_q27.json, tools/capture_lattices.py), and every refusal -- in the simulation classes and, through
tests/lat_bind_main.cpp, in the library's module configuration and kernel table."""
import itertools
import json
import os
import re

import pytest

from sailfish_amd import hipabi, sym
from tests import _bind, _host, _lat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sailfish_amd', 'csrc')


@pytest.fixture(scope='module')
def tables(golden_dir):
    with open(os.path.join(golden_dir, 'lattices_q15_q27.json')) as fh:
        return json.load(fh)


# ---- tables -------------------------------------------------------------------------------------------------------------

def test_known_grids_and_the_default():
    assert [g.__name__ for g in sym.KNOWN_GRIDS] == ['D2Q9', 'D3Q19', 'D3Q15', 'D3Q27']
    assert [g.__name__ for g in sym.KNOWN_GRIDS if g.dim == 3][0] == 'D3Q19'          # the default --grid in 3-D
    assert sym.lookup_grid('D3Q15') is sym.D3Q15 and sym.lookup_grid('D3Q27') is sym.D3Q27
    with pytest.raises(ValueError, match='D3Q13.*D3Q15 and D3Q27'):
        sym.lookup_grid('D3Q13')
    assert (hipabi.SLF_D3Q15, hipabi.SLF_D3Q27) == (2, 3) == (sym.D3Q15.slf_id, sym.D3Q27.slf_id)


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_host_tables(tables, name):
    grid, t = sym.lookup_grid(name), tables[name]
    assert grid.dim == t['dim'] and grid.Q == t['Q']
    assert [list(e) for e in grid.basis] == t['basis']
    assert [w.numerator for w in grid.weights] == t['weights_num']
    assert [w.denominator for w in grid.weights] == t['weights_den']
    assert sum(grid.weights) == 1
    assert grid.idx_name == t['idx_name']
    assert grid.idx_opposite == t['idx_opposite']
    assert {str(k): v for k, v in grid.dir2vecidx.items()} == t['dir2vecidx']
    for o in range(1, 7):
        assert sym.get_missing_dists(grid, o) == t['missing_dists'][str(o)]
    for axis in range(3):
        for d in (-1, 0, 1):
            assert sym.get_prop_dists(grid, d, axis) == t['prop_dists']['%d_%d' % (axis, d)]
    for d in itertools.product((-1, 0, 1), repeat=3):
        if any(d):
            key = ','.join(str(c) for c in d)
            assert sym.get_interblock_dists(grid, d) == t['interblock_dists'][key]['normal']
            assert sym.get_interblock_dists(grid, d, opposite=True) == t['interblock_dists'][key]['opposite']
    # no MRT here, whatever the reference has; only the BGK collision is served
    assert not hasattr(grid, 'mrt_matrix')
    assert grid.model_supported('bgk') and not grid.model_supported('mrt') and not grid.model_supported('elbm')
    assert sym.mrt_rates(grid, 0.1) == [0.0] * grid.Q


def test_interblock_known_answers_of_the_issue():
    assert sym.get_interblock_dists(sym.D3Q15, (1, 1, 0)) == [7, 11]
    assert sym.get_interblock_dists(sym.D3Q15, (1, 1, 1)) == [7]
    assert len(sym.get_interblock_dists(sym.D3Q27, (1, 0, 0))) == 9
    assert sym.get_interblock_dists(sym.D3Q27, (1, 1, 0)) == [7, 19, 20]


def _c_ternary(expr):
    """A C conditional expression over `i` and integers as a Python one."""
    expr = expr.strip()
    while expr.startswith('(') and expr.endswith(')') and _balanced(expr[1:-1]):
        expr = expr[1:-1].strip()
    depth = 0
    for k, ch in enumerate(expr):
        depth += ch == '('
        depth -= ch == ')'
        if ch == '?' and depth == 0:
            colon, nest, d2 = None, 0, 0
            for j in range(k + 1, len(expr)):
                d2 += expr[j] == '('
                d2 -= expr[j] == ')'
                if d2 == 0 and expr[j] == '?':
                    nest += 1
                if d2 == 0 and expr[j] == ':':
                    if nest == 0:
                        colon = j
                        break
                    nest -= 1
            return '(%s if %s else %s)' % (_c_ternary(expr[k + 1:colon]), expr[:k].strip(), _c_ternary(expr[colon + 1:]))
    return expr


def _balanced(s):
    depth = 0
    for ch in s:
        depth += ch == '('
        depth -= ch == ')'
        if depth < 0:
            return False
    return depth == 0


def header_tables(name):
    """struct `name` of csrc/slf_lattice.h: its Q, id, the arrays of ex / ey / ez / opp and the weight expressions."""
    src = open(os.path.join(CSRC, 'slf_lattice.h')).read()
    body = src[src.index('struct %s {' % name):]
    body = body[:body.index('\n};')]
    out = {k: int(re.search(r'static constexpr int %s = (\d+);' % k, body).group(1)) for k in ('dim', 'Q', 'id')}
    for fn in ('ex', 'ey', 'ez', 'opp'):
        m = re.search(r'static constexpr int %s\(int i\) \{\s*constexpr int t\[(\d+)\] = \{([^}]*)\};' % fn, body)
        assert int(m.group(1)) == out['Q']
        out[fn] = [int(x) for x in m.group(2).split(',')]
    for fn in ('wnum', 'wden'):
        expr = _c_ternary(re.search(r'static constexpr int %s\(int ?i?\) \{ return ([^;]*); \}' % fn, body).group(1))
        out[fn] = [int(eval(expr, {'i': i})) for i in range(out['Q'])]
    out['dir2vecidx'] = re.search(r'static constexpr int dir2vecidx\(int o\) \{ return ([^;]*); \}', body).group(1)
    out['has_mrt'] = 'mrt' in body.split('//')[0] or bool(re.search(r'static constexpr int mrt', body))
    return out


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_header_tables(tables, name):
    t, h = tables[name], header_tables(name)
    assert (h['dim'], h['Q'], h['id']) == (t['dim'], t['Q'], sym.lookup_grid(name).slf_id)
    assert [[x, y, z] for x, y, z in zip(h['ex'], h['ey'], h['ez'])] == t['basis']
    assert h['opp'] == t['idx_opposite']
    assert h['wnum'] == t['weights_num'] and h['wden'] == t['weights_den']
    assert h['dir2vecidx'] == 'o' and t['dir2vecidx'] == {str(o): o for o in range(1, 7)}
    assert not h['has_mrt']


def test_header_reader_on_the_lattice_it_already_pins(golden_dir):
    """The reader itself, on D3Q19, against tests/golden/lattices.json."""
    with open(os.path.join(golden_dir, 'lattices.json')) as fh:
        t = json.load(fh)['D3Q19']
    h = header_tables('D3Q19')
    assert [[x, y, z] for x, y, z in zip(h['ex'], h['ey'], h['ez'])] == t['basis']
    assert h['opp'] == t['idx_opposite'] and h['wnum'] == t['weights_num'] and h['wden'] == t['weights_den']


# ---- refusals on the host -------------------------------------------------------------------------------------------------

def _desc(sim_cls, cfg, geo=None):
    from sailfish_amd.geo import LBGeometry3D
    _, _, runners = _host.build_runners(sim_cls, 3, geo or LBGeometry3D, cfg)
    r = runners[0]
    r._init_geometry()
    r._sim.init_fields(r)
    r._subdomain.init_fields(r._sim)
    return r, r._module_desc()


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_what_is_served_builds_a_descriptor(name):
    sim, cfg = _lat.case(name, _lat.CHANNEL, pattern='AA', precision='single', incompressible=True)
    r, d = _desc(sim, cfg)
    assert d.lattice == sym.lookup_grid(name).slf_id and d.model == hipabi.SLF_BGK and d.has_force == 1
    assert int(d.force_implementation) == hipabi.SLF_FORCE_EDM and int(d.incompressible) == hipabi.SLF_DENSITY_INCOMPRESSIBLE
    assert hipabi.SLF_NK_HALF_BB in list(d.type_kind[:d.n_types])
    from sailfish_amd.backend_hip import HIPBackend
    assert not HIPBackend.supports_row_classes(d)


HOST_REFUSALS = [
    (dict(model='mrt'), 'mrt'),
    (dict(model='elbm'), 'elbm'),
    (dict(regularized=True), 'regularized'),
    (dict(subgrid='les-smagorinsky', smagorinsky_const=0.1), 'subgrid'),
    (dict(minimize_roundoff=True), 'minimize_roundoff'),
    (dict(node_addressing='indirect'), 'indirect'),
]


@pytest.mark.parametrize('over,word', HOST_REFUSALS, ids=[w for _, w in HOST_REFUSALS])
@pytest.mark.parametrize('name', _lat.LATTICES)
def test_options_refused_by_name(name, over, word):
    sim, cfg = _lat.case(name, _lat.PERIODIC_BOX)
    cfg.update(over)
    with pytest.raises((ValueError, NotImplementedError), match='(%s.*%s)|(%s.*%s)' % (word, name, name, word)):
        _desc(sim, cfg)


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_other_node_types_refused_by_name(name):
    from sailfish_amd.node_type import NTEquilibriumVelocity
    from sailfish_amd.subdomain import Subdomain3D
    from sailfish_amd.lb_single import LBFluidSim

    class Box(Subdomain3D):
        def boundary_conditions(self, hx, hy, hz):
            self.set_node(hz == 0, NTEquilibriumVelocity((0.01, 0.0, 0.0)))

        def initial_conditions(self, sim, hx, hy, hz):
            sim.rho[:] = 1.0

    class Sim(LBFluidSim):
        subdomain = Box

    with pytest.raises(NotImplementedError, match='%s: NTEquilibriumVelocity is not served; fluid, NTFullBBWall and NTHalfBBWall nodes only' % name):
        _desc(Sim, _lat.config(name, (8, 6, 6), walls='full'))


def _models():
    from sailfish_amd.lb_binary import LBBinaryFluidFreeEnergy, LBBinaryFluidShanChen
    from sailfish_amd.lb_single import LBSingleFluidShanChen
    from sailfish_amd.lb_ternary import LBTernaryFluidShanChen
    return [LBSingleFluidShanChen, LBBinaryFluidShanChen, LBBinaryFluidFreeEnergy, LBTernaryFluidShanChen]


@pytest.mark.parametrize('model', range(4), ids=['shan-chen-single', 'shan-chen-binary', 'free-energy', 'ternary'])
@pytest.mark.parametrize('name', _lat.LATTICES)
def test_other_models_refused_by_name(name, model):
    from sailfish_amd.subdomain import Subdomain3D
    base = _models()[model]

    class Box(Subdomain3D):
        def boundary_conditions(self, hx, hy, hz):
            pass

        def initial_conditions(self, sim, hx, hy, hz):
            for f in ('rho', 'phi', 'theta'):
                if hasattr(sim, f):
                    getattr(sim, f)[:] = 1.0

    class Sim(base):
        subdomain = Box

    cfg = _lat.config(name, (8, 6, 6), G=1.0, G11=0.0, G12=1.0, G13=1.0, G22=0.0, G23=1.0, G33=0.0, sc_potential='linear', tau_phi=1.0,
                      tau_theta=1.0, Gamma=0.5, kappa=0.04, A=0.04, tau_a=1.0, tau_b=1.0, bc_wall_grad_phase=0.0,
                      bc_wall_grad_order=2, model='bgk')
    offender = ('the Shan-Chen models are', 'the Shan-Chen models are', 'the free-energy model is', 'the ternary Shan-Chen model is')[model]
    with pytest.raises(NotImplementedError, match='%s: %s not served; single-fluid modules only' % (name, offender)):
        _desc(Sim, cfg)


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_force_objects_refused_by_name(name):
    from sailfish_amd.lb_base import ForceObject
    sim, cfg = _lat.case(name, _lat.WALL_BOX)
    r, d = _desc(sim, cfg)
    r._desc = d
    r._sim.add_force_object(ForceObject((2, 2, 2), (5, 5, 5)))
    with pytest.raises(NotImplementedError, match='%s: force objects' % name):
        r._init_force_objects()


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_x_face_buffers_and_planes_stay_d3q19(name):
    """The x-face buffers and planes are guarded by Q == 19: a slab of these lattices goes through ghost columns and lists."""
    src = open(os.path.join(ROOT, 'sailfish_amd', 'xface.py')).read()
    assert src.count('grid.Q == 19') >= 2
    sim, cfg = _lat.case(name, _lat.PERIODIC_BOX)
    r, d = _desc(sim, dict(cfg, subdomains=2, conn_axis='x'), geo='EqualSubdomainsGeometry3D')
    assert d.lattice == sym.lookup_grid(name).slf_id


# ---- refusals in the library (slf_bind.h), as a stand-alone program ---------------------------------------------------------

@pytest.fixture(scope='module')
def bind_lines(tmp_path_factory):
    done = _bind.run('lat_bind_main.cpp', tmp_path_factory.mktemp('lat_bind'))
    assert done.returncode == 0, done.stderr[-4000:]
    return [ln.split('\t') for ln in done.stdout.splitlines()]


OK, INVALID, UNSUPPORTED, NOT_FOUND = 0, 1, 3, 4
CONFIG_WORDS = {'mrt': 'model=mrt', 'elbm': 'model=elbm', 'regularized': 'regularized', 'subgrid': 'subgrid',
                'minimize_roundoff': 'minimize_roundoff', 'indirect': 'indirect', 'shan-chen-binary': 'Shan-Chen',
                'shan-chen-single': 'Shan-Chen', 'free-energy': 'free-energy', 'ternary': 'ternary'}
# kernel kinds (slf::KernelKind) a module of these lattices serves: the four of slf_lat.hip and the kernels that never look
# at a direction (macro-field ghost fill, index-list and box pack / unpack)
SERVED = {'CollideAndPropagate': 0, 'SetInitialConditions': 1, 'ApplyPeriodicBoundaryConditions': 2,
          'ApplyPeriodicBoundaryConditionsWithSwap': 3, 'ApplyMacroPeriodicBoundaryConditions': 4, 'CollectSparseData': 5,
          'DistributeSparseData': 6, 'CollectContinuousData': 7, 'DistributeContinuousData': 8, 'ComputeMacroFields': 13}


def test_error_codes_are_the_headers():
    src = open(os.path.join(ROOT, 'include', 'sailfish_hip.h')).read()
    for name, val in (('SLF_OK', OK), ('SLF_ERR_INVALID', INVALID), ('SLF_ERR_NOT_FOUND', NOT_FOUND), ('SLF_ERR_UNSUPPORTED', UNSUPPORTED)):
        assert re.search(r'%s\s*=\s*%d\b' % (name, val), src), name


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_module_configuration(bind_lines, name):
    rows = {ln[2]: ln for ln in bind_lines if ln[0] == 'config' and ln[1] == name}
    for subject in ('served', 'served-aa-f64-force-edm-incompressible'):
        assert int(rows[subject][3]) == OK, rows[subject]
        assert rows[subject][5] == 'variant=0'          # routed around the tuned D3Q19 kernels
    for subject, word in CONFIG_WORDS.items():
        code, msg = int(rows[subject][3]), rows[subject][4]
        assert code == UNSUPPORTED and msg.startswith(name + ': ') and word in msg, rows[subject]
    kinds = [s for s in rows if s.startswith('node-kind-')]
    assert len(kinds) == 11          # SLF_NK_REGULARIZED_VELOCITY .. SLF_NK_WALL_TMS
    for s in kinds:
        assert int(rows[s][3]) == UNSUPPORTED and re.match(name + r': NT\w+ is not served; fluid, NTFullBBWall and NTHalfBBWall nodes only$', rows[s][4]), rows[s]


def test_unknown_lattices_stay_unknown(bind_lines):
    rows = [ln for ln in bind_lines if ln[0] == 'config' and ln[2] == 'unknown']
    assert len(rows) == 2 and all(int(ln[3]) == UNSUPPORTED and ln[4] == 'unsupported lattice' for ln in rows)


@pytest.mark.parametrize('name', _lat.LATTICES)
def test_every_kernel_name_is_served_by_lattice_aware_code_or_refused(bind_lines, name):
    rows = [ln for ln in bind_lines if ln[0] == 'resolve' and ln[1] == name]
    table = set(re.findall(r'^  \{"(\w+)", KK_', open(os.path.join(CSRC, 'slf_bind.h')).read(), re.M))
    assert len(table) >= 25 and set(ln[2].rsplit('-', 1)[0] for ln in rows) == table
    for ln in rows:
        kernel, access = ln[2].rsplit('-', 1)
        code, msg, kind = int(ln[3]), ln[4], int(ln[5])
        if kernel in SERVED and not (kernel.endswith('WithSwap') and access == 'ab'):
            assert code == OK and kind == SERVED[kernel], ln
        else:
            assert code in (NOT_FOUND, UNSUPPORTED) and msg, ln
            if code == UNSUPPORTED:
                assert name in msg, ln
    refused = dict((ln[2], ln[4]) for ln in rows if int(ln[3]) != OK)
    assert name in refused['CollideAndPropagateResident-ab']
    for k in ('CollectContinuousDataWithSwap-aa', 'DistributeContinuousDataWithSwap-aa', 'CollectContinuousMacroData-ab',
              'DistributeContinuousMacroData-aa'):
        assert name in refused[k] and 'face argument lists' in refused[k]
    binds = [ln for ln in bind_lines if ln[0] == 'bind' and ln[1] == name]
    assert len(binds) == 2 and all(int(ln[3]) == UNSUPPORTED and 'D3Q15 / D3Q27' in ln[4] for ln in binds)
