"""Force objects on the GPU: the kernel (sailfish_amd/csrc/slf_force.hip) through HIPBackend on random arrays and random
link tables, the public surface through LBSimulationController, and examples/square_cylinder_2d.py.

Sums are compared with math.fsum of the twin's terms (tests/_force_twin.py: the bracket of a link formed in the module's
precision, times -1 / 0 / 1) under the bound of any summation order, |got - fsum(t)| <= n 2^-53 sum|t| per component, as
in tests/test_gpu_stats.py: the twin's terms ARE the kernel's terms, the order of addition is the only difference.
Nothing here is sized from what the kernel returns."""
import numpy as np
import pytest

from sailfish_amd import hipabi, sym
from sailfish_amd.box import make_box_desc
from tests import _force_sims as fs
from tests import _force_twin as tw

pytestmark = pytest.mark.gpu

DTYPE = {'single': np.float32, 'double': np.float64}
GRIDS = {'D2Q9': (sym.D2Q9, (20, 12)), 'D3Q19': (sym.D3Q19, (20, 12, 9))}
# links of the first and the last of three objects (the middle one is empty): one link; below, at and above a wave; below, at
# and above a chunk of hipabi.SLF_FORCE_CHUNK links (above it: partial sums and a second launch); 5000
COUNTS = [(1, 63), (64, 65), (0, 5000), (5000, 1), (hipabi.SLF_FORCE_CHUNK, hipabi.SLF_FORCE_CHUNK + 1)]


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


class Call(object):
    """Random populations, random link tables of three objects, and the device side of one slf_force_objects call."""

    def __init__(self, backend, grid_name, precision, counts, seed):
        self.b, (self.grid, size) = backend, GRIDS[grid_name]
        self.desc = make_box_desc(self.grid, size, precision=precision)
        self.module = backend.build(self.desc)
        self.words = self.grid.Q * hipabi.dist_stride(self.desc)
        rng = self.rng = np.random.RandomState(seed)
        self.dist = (0.05 + 0.02 * rng.standard_normal(self.words)).astype(DTYPE[precision])
        self.links = [self.random_links(n) for n in (counts[0], 0, counts[1])]
        first = [l for l in self.links if len(l[0])][0]
        last = [l for l in self.links if len(l[0])][-1]
        first[0][0] = 0                         # the first and the last word of the array
        last[1][-1] = self.words - 1
        self.stream = backend.make_stream()
        self.gpu_dist = backend.alloc_buf(like=self.dist)
        self._bufs = [self.gpu_dist]

    def random_links(self, n):
        return [self.rng.randint(0, self.words, n).astype(np.uint32), self.rng.randint(0, self.words, n).astype(np.uint32),
                self.rng.randint(1, self.grid.Q, n).astype(np.uint8)]

    def run(self):
        """One call on the current self.links -> [objects, 3] doubles."""
        b = self.b
        idx, idx2, dirs = [np.concatenate([l[k] for l in self.links]) for k in range(3)]
        seg = np.cumsum([0] + [len(l[0]) for l in self.links]).astype(np.uint32)
        assert max(int(idx.max()), int(idx2.max())) < self.words            # the device does not check
        n, longest = len(self.links), int(np.diff(seg).max())
        out = np.full(3 * n, np.nan)
        bufs = [b.alloc_buf(like=a) for a in (idx, idx2, dirs, seg, out)]
        ws = b.force_workspace(self.module, n, longest)
        assert (ws != 0) == (longest > hipabi.SLF_FORCE_CHUNK)
        b.force_objects(self.module, self.gpu_dist, bufs[0], bufs[1], bufs[2], bufs[3], n, longest, ws, bufs[4], self.stream)
        self.stream.synchronize()
        b.from_buf(bufs[4])
        for a in bufs + ([ws] if ws else []):
            b.free_buf(a)
        return out.reshape(n, 3).copy()

    def close(self):
        for a in self._bufs:
            self.b.free_buf(a)


@pytest.mark.parametrize('counts', COUNTS, ids=lambda c: '%d_0_%d' % c)
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('grid_name', sorted(GRIDS))
def test_kernel_on_random_tables(backend, grid_name, precision, counts):
    c = Call(backend, grid_name, precision, counts, seed=7 + counts[0])
    try:
        got = c.run()
        for o, (idx, idx2, dirs) in enumerate(c.links):
            t = tw.link_terms(c.dist, idx, idx2, dirs, c.grid)
            want, tol = tw.fsum_force(t), tw.bound(t)
            for k in range(3):
                print('object %d component %d: got %.17g fsum %.17g bound %.3g' % (o, k, got[o, k], want[k], tol[k]))
                assert abs(got[o, k] - want[k]) <= tol[k], (o, k)
            if c.grid.dim == 2 or not len(idx):
                assert got[o, 2] == 0.0
        assert np.array_equal(got[1], np.zeros(3))                  # the empty object in the middle
        again = c.run()
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64))     # the same bits, call after call
        # other links for the first object (another count as well): the other objects keep their bits
        c.links[0] = c.random_links(len(c.links[0][0]) + 37)
        other = c.run()
        assert np.array_equal(other[1:].view(np.uint64), got[1:].view(np.uint64))
        assert not np.array_equal(other[0], got[0])
    finally:
        c.close()


# ---- through the controller on the device --------------------------------------------------------------------------------
CASES = {'cylinder': (fs.cylinder_sim, 2, fs.CYLINDER, fs.CYLINDER_BOX), 'sphere': (fs.sphere_sim, 3, fs.SPHERE, fs.SPHERE_BOX)}
SAMPLE_AT = (40, 41)        # steps completed: both parities of the in-place pattern


def _run(name, precision, pattern, addressing):
    """{steps completed: (fo.force(), twin terms on _debug_get_dist())} of one run of 41 steps."""
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    simf, dim, base, box = CASES[name]
    out = {}

    def hook(sim, runner):
        if sim.iteration not in SAMPLE_AT:
            return
        fo = sim.force_objects[0]
        runner.update_force_objects()
        runner.backend.from_buf(fo.gpu_force_buf)
        got = fo.force()
        real = runner._debug_get_dist()[(slice(None),) + tuple(runner._spec._nonghost_slice)]
        odd = pattern == 'AA' and (sim.iteration & 1) == 1
        terms = tw.force_terms_on_box(real, runner._subdomain.visualization_map(), runner._spec.location, box[0], box[1],
                                      sim.grid, odd)
        assert terms.shape[0] == fo.num_links and real.dtype == DTYPE[precision]
        out[sim.iteration] = (got, terms)

    ctrl = LBSimulationController(simf(hook=hook), getattr(geo_mod, 'EqualSubdomainsGeometry%dD' % dim),
                                  default_config=dict(base, max_iters=max(SAMPLE_AT), quiet=True, perf_stats_every=0, gpus=[0],
                                                      output='', access_pattern=pattern, node_addressing=addressing,
                                                      precision=precision))
    ctrl.run(ignore_cmdline=True)
    for r in ctrl.runners:
        r.release()
    assert sorted(out) == list(SAMPLE_AT)
    return out


@pytest.fixture(scope='module')
def runs():
    cache = {}

    def get(name, precision, pattern, addressing):
        key = (name, precision, pattern, addressing)
        if key not in cache:
            cache[key] = _run(*key)
        return cache[key]
    return get


@pytest.mark.parametrize('addressing', ['direct', 'indirect'])
@pytest.mark.parametrize('pattern', ['AB', 'AA'])
@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_force_through_the_controller_equals_the_twin(runs, name, precision, pattern, addressing):
    res = runs(name, precision, pattern, addressing)
    dim = CASES[name][1]
    for it in SAMPLE_AT:
        got, terms = res[it]
        want, tol = tw.fsum_force(terms), tw.bound(terms)
        assert len(got) == dim
        for k in range(dim):
            print('%d steps, component %d: got %.17g fsum %.17g bound %.3g' % (it, k, got[k], want[k], tol[k]))
            assert abs(got[k] - want[k]) <= tol[k], (it, k)
        assert got[0] > 0           # the body is pushed along the flow


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_patterns_and_addressing_modes_give_the_same_bits(runs, name, precision):
    ref = runs(name, precision, 'AB', 'direct')
    for pattern, addressing in (('AA', 'direct'), ('AB', 'indirect'), ('AA', 'indirect')):
        res = runs(name, precision, pattern, addressing)
        for it in SAMPLE_AT:
            assert res[it][0] == ref[it][0], (pattern, addressing, it)


# ---- the example ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wall', ['halfbb', 'fullbb'])
def test_square_cylinder_example(wall):
    """H = 24: the smallest channel whose cylinder has an edge of 3 (D = int(0.02 int(6.25 H))).  400 steps, sampled every
    100: finite forces, drag along the flow.  The lift is small against the drag: zero by symmetry where the cylinder's
    node layers can be centred (full-way walls: 2 layers in 26 rows); the 5 layers of the half-way walls in 24 rows sit half
    a spacing off the axis, 1 / 48 of the channel height, and the lift of a body slightly off the axis of a channel grows
    linearly with the offset from zero -- a few per cent of the drag, bounded here by 10 %."""
    from examples.square_cylinder_2d import SquareCylinderSim
    from sailfish_amd.controller import LBSimulationController
    ctrl = LBSimulationController(SquareCylinderSim, default_config=dict(H=24, wall=wall, force_every=100, max_iters=400,
                                                                         quiet=True, perf_stats_every=0, output='', gpus=[0]))
    ctrl.run(ignore_cmdline=True)
    sim = ctrl.runners[0]._sim
    for r in ctrl.runners:
        r.release()
    assert sim.D == 3 and sim.force_objects[0].initialized and sim.force_objects[0].num_links > 0
    assert [s[0] for s in sim.samples] == [100, 200, 300, 400]
    s = np.array(sim.samples)
    print(s)
    assert np.isfinite(s).all()
    assert (s[:, 3] > 0).all()
    assert (np.abs(s[:, 4]) < 0.1 * s[:, 3]).all()
    if wall == 'fullbb':
        assert (np.abs(s[:, 4]) < 1e-9 * s[:, 3]).all()
