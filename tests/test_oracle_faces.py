"""The CPU oracle is frame-invariant: a channel with its flow along any axis, in either sense, with its walls on any
other axis (tests/_faces.py) is the same flow as in the x frame.  Every frame's density and velocity, carried back to
the x frame, agree with the x-frame run within 1e-12 in double precision (measured: at most 1.1e-14 in D3Q19, 5.2e-15
in D2Q9; an outlet that faces the wrong way moves the fields by 0.07 or fills them with the ghost nodes' non-finite
values -- asserted below, so the bound does separate right from wrong).  This is what makes bit-identity of a kernel
with the oracle in a frame (tests/test_gpu_faces.py) mean that the kernel is right there."""
import numpy as np
import pytest

from sailfish_amd import sym
from sailfish_amd.box import make_box_desc
from tests import _faces as F
from tests import _geometry as geo
from tests._oracle_box import OracleBox

TOL = 1e-12
STEPS = (40, 41)


def run_oracle(grid, frame, case, size, steps, **kw):
    """-> (rho, [v...]) on the real nodes in the x frame, and the mask of the fluid nodes there."""
    periodic, node_map_fn, (rho, v), dkw = F.setup(grid, frame, case, size, **kw)
    desc = make_box_desc(grid, size, **dkw)
    nmap = node_map_fn(desc)
    o = OracleBox(desc, periodic=periodic, node_map=nmap)
    o.set_fields(rho, v)
    o.initial_conditions()
    o.run(steps, save_last=True)
    fields = F.to_x_frame((o.real_view(o.rho).copy(), [o.real_view(o.v[d]).copy() for d in range(grid.dim)]), frame)
    fluid = (o.real_view(nmap) & ((1 << geo.NT_BITS[0]) - 1)) == geo.T_FLUID
    return fields, F.scalar_to_x_frame(fluid, frame)


def _size(grid, frame):
    return F.size_of(frame, 14, 8, 5 if grid.dim == 3 else None)


def _cases(grid):
    return F.CASES_3D + F.EXTRA_3D if grid.dim == 3 else F.CASES_2D


_x_runs = {}


def x_frame_run(grid, case, steps):
    key = (grid.dim, case, steps)
    if key not in _x_runs:
        frame = F.X_FRAME[grid.dim]
        _x_runs[key] = run_oracle(grid, frame, case, _size(grid, frame), steps, precision='double')
    return _x_runs[key]


def _deviation(got, ref):
    dev = 0.0
    for g, r in zip([got[0]] + got[1], [ref[0]] + ref[1]):
        fin = np.isfinite(r)
        assert np.array_equal(fin, np.isfinite(g))
        dev = max(dev, float(np.max(np.abs(g[fin] - r[fin]))))
    return dev


@pytest.mark.parametrize('grid', [sym.D3Q19, sym.D2Q9], ids=['D3Q19', 'D2Q9'])
def test_frames_cover_every_face(grid):
    fr = F.frames(grid.dim)
    assert len(fr) == len(set(fr)) == (12 if grid.dim == 3 else 4)
    assert F.X_FRAME[grid.dim] in fr
    # inlet normals: every one of the 2 dim faces, each as often as any other
    normals = [grid.vec_to_dir(F.vec_from_x_frame((1, 0, 0)[:grid.dim], f)) for f in fr]
    assert sorted(set(normals)) == list(range(1, 2 * grid.dim + 1))
    assert len(set(normals.count(n) for n in set(normals))) == 1


@pytest.mark.parametrize('grid', [sym.D3Q19, sym.D2Q9], ids=['D3Q19', 'D2Q9'])
def test_to_x_frame_inverts_from_x_frame(grid):
    rng = np.random.RandomState(3)
    shape = (5, 8, 14)[3 - grid.dim:]
    rho = rng.rand(*shape)
    for frame in F.frames(grid.dim):
        a, s, b, c = F.axes(frame)
        there = F.from_x_frame(rho, frame)
        assert there.shape == tuple(reversed(F.size_of(frame, 14, 8, 5 if grid.dim == 3 else None)))
        v = [None] * grid.dim
        v[a], v[b] = s * there, 2 * there
        if c is not None:
            v[c] = 3 * there
        back, vb = F.to_x_frame((there, v), frame)
        assert np.array_equal(back, rho)
        for k, comp in enumerate(vb):
            assert np.array_equal(comp, (k + 1) * rho)


def _case_params():
    out = []
    for grid, name in ((sym.D3Q19, 'D3Q19'), (sym.D2Q9, 'D2Q9')):
        for case in _cases(grid):
            out.append(pytest.param(grid, case, id='%s-%s' % (name, F.case_id(case))))
    return out


@pytest.mark.parametrize('grid,case', _case_params())
def test_oracle_is_frame_invariant(grid, case):
    worst = 0.0
    for steps in STEPS:
        ref, ref_fluid = x_frame_run(grid, case, steps)
        assert np.all(np.isfinite(ref[0][ref_fluid])), 'x frame: non-finite fluid nodes'
        for frame in F.frames(grid.dim):
            got, fluid = run_oracle(grid, frame, case, _size(grid, frame), steps, precision='double')
            assert np.array_equal(fluid, ref_fluid), F.frame_id(frame)
            for field in [got[0]] + got[1]:
                assert np.all(np.isfinite(field[fluid])), F.frame_id(frame)
            dev = _deviation(got, ref)
            assert dev < TOL, (F.frame_id(frame), steps, dev)
            worst = max(worst, dev)
        # the boundary did something: the speed along the flow is not uniform over the layer it acts on
        layer = F.outlet_layer(ref[1][0], F.X_FRAME[grid.dim], case[0])
        assert np.ptp(layer[np.isfinite(layer)]) > 0
    print('%s %s: largest frame deviation %.2e' % (grid.__name__, F.case_id(case), worst))


@pytest.mark.parametrize('grid', [sym.D3Q19, sym.D2Q9], ids=['D3Q19', 'D2Q9'])
@pytest.mark.parametrize('case', [c for c in F.CASES_3D if c[0] in F.OPEN and c[3] == 'single' or c[0] == 'eq'],
                         ids=F.case_id)
def test_an_outlet_that_faces_the_wrong_way_is_seen(grid, case):
    """The outlet encoded with the inlet's normal: far outside the tolerance of the frame test, or non-finite on a
    fluid node.  One case per outlet kind: Zou-He, regularized and equilibrium density, copy, Yu, do-nothing."""
    frame = F.X_FRAME[grid.dim]
    seen = set()
    for steps in STEPS:
        ref, ref_fluid = x_frame_run(grid, case, steps)
        got, fluid = run_oracle(grid, frame, case, _size(grid, frame), steps, precision='double',
                                out_normal=(1, 0, 0))
        assert np.array_equal(fluid, ref_fluid)
        bad = False
        dev = 0.0
        for g, r in zip([got[0]] + got[1], [ref[0]] + ref[1]):
            if not np.all(np.isfinite(g[fluid])):
                bad = True
            else:
                dev = max(dev, float(np.max(np.abs(g[fluid] - r[fluid]))))
        assert bad or dev > 1e-4, (steps, dev)
        seen.add('non-finite' if bad else 'moved')
    print('%s %s: %s' % (grid.__name__, F.case_id(case), sorted(seen)))
