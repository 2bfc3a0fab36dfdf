"""The statistics kernels (sailfish_amd/csrc/slf_stats.hip) on the GPU: through the backend against their numpy twin
(tests/_stats_twin.py, itself held against the reference by tests/test_stats_host.py), and through the controller with
the two mix-ins of sailfish.stats.

Per-node values are compared bit for bit.  Sums are compared with math.fsum of the twin's terms under the bound of any
summation order, |got - fsum(t)| <= n 2^-53 sum|t| (+ |result| 2^-53 per division that follows): the twin's terms ARE
the kernel's terms, so the order of addition is the only difference.  Nothing here is sized from what the kernels
return."""
import numpy as np
import pytest

from sailfish_amd import hipabi, sym
from sailfish_amd.box import make_box_desc
from tests import _geometry as geo
from tests import _stats_twin as tw

pytestmark = pytest.mark.gpu

# (nx, ny, nz): row shorter than a wave; several waves, no multiple of 64; row longer than a workgroup + extent 2;
# every axis at extent 2
SHAPES = [(20, 12, 9), (130, 5, 3), (1100, 3, 2), (2, 2, 2)]
DTYPE = {'single': np.float32, 'double': np.float64}


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def _random_fields(size, dtype, seed):
    """rho around 1, velocities of both signs: [nz, ny, nx] / [3, nz, ny, nx]."""
    rng = np.random.RandomState(seed)
    shape = tuple(reversed(size))
    rho = (1.0 + 0.1 * rng.standard_normal(shape)).astype(dtype)
    v = (0.1 * rng.standard_normal((3,) + shape)).astype(dtype)
    return rho, v


class Device(object):
    """A module of the given box and the device copies of its fields, ghost layer (and x padding) at +inf."""

    def __init__(self, backend, size, precision, node_map=False):
        self.b = backend
        self.size = size
        self.dtype = DTYPE[precision]
        kw = dict(fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS) if node_map else {}
        self.desc = make_box_desc(sym.D3Q19, size, precision=precision, **kw)
        self.module = backend.build(self.desc)
        self.shape = (self.desc.arr_nz, self.desc.arr_ny, self.desc.arr_nx)
        self.stream = backend.make_stream()
        self.off = backend.dist_align_offset(self.dtype().itemsize)
        self.sums = np.zeros(2)
        self.gpu_sums = backend.alloc_buf(like=self.sums)
        self.ke_ws = backend.stats_workspace(self.module, hipabi.SLF_STATS_KE_ENSTROPHY)
        self._bufs = [self.gpu_sums, self.ke_ws]

    def real(self, full):
        nx, ny, nz = self.size
        return full[1:nz + 1, 1:ny + 1, 1:nx + 1]

    def field(self, values=None, fill=np.inf):
        """Host array in the module's layout + its device copy; `values` go to the real nodes."""
        host = np.full(self.shape, fill, dtype=self.dtype)
        if values is not None:
            self.real(host)[...] = values
        addr = self.b.alloc_buf(like=host, align_offset=self.off)
        self._bufs.append(addr)
        return host, addr

    def map(self, unused):
        m = geo.empty_map(self.desc)
        self.real(m)[unused] = geo.encode(geo.T_UNUSED)
        addr = self.b.alloc_buf(like=m, align_offset=self.b.dist_align_offset(4))
        self._bufs.append(addr)
        return addr

    def ke(self, gpu_v, gpu_map=0, out=(0, 0)):
        self.b.stats_ke_enstrophy(self.module, gpu_map, gpu_v, self.ke_ws, self.gpu_sums, out[0], out[1], self.stream)
        self.b.from_buf_async(self.gpu_sums, self.stream)
        self.stream.synchronize()
        return self.sums.copy()

    def fetch(self, host, addr):
        self.b.from_buf(addr, host)
        return host

    def release(self):
        self.stream.synchronize()
        for a in self._bufs:
            self.b.free_buf(a)


def _within(got, terms, what):
    ref, bound = tw.sum_and_bound(terms)
    print('%s: got %.17g, fsum %.17g, |diff| %.3e, bound %.3e' % (what, got, ref, abs(got - ref), bound))
    assert abs(got - ref) <= bound, what


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('size', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('flow', ['kida', 'random'])
def test_ke_enstrophy_kernel(backend, flow, size, precision):
    dtype = DTYPE[precision]
    v = tw.kida(size, 0.05, dtype) if flow == 'kida' else _random_fields(size, dtype, 11)[1]
    d = Device(backend, size, precision)
    try:
        gpu_v = [d.field(c)[1] for c in v]
        h_vsq, g_vsq = d.field(fill=np.nan)               # whatever the arrays held: the kernel writes every entry
        h_wsq, g_wsq = d.field(fill=np.nan)
        sums = d.ke(gpu_v, out=(g_vsq, g_wsq))
        want_vsq, want_wsq = tw.ke_fields(v)
        for host, addr, want, name in ((h_vsq, g_vsq, want_vsq, 'v_sq'), (h_wsq, g_wsq, want_wsq, 'vort_sq')):
            got = d.fetch(host, addr)
            assert np.array_equal(d.real(got), want), name           # bit for bit (no ghost value got in: they are +inf)
            ghost = np.ones(d.shape, dtype=bool)
            d.real(ghost)[...] = False
            ghost[:, :, d.desc.lat_nx:] = False                      # (x padding beyond the lattice box: not the kernel's)
            assert np.all(got[ghost] == 0), name + ' ghost layer'
        _within(sums[0], want_vsq, 'sum v_sq')
        _within(sums[1], want_wsq, 'sum vort_sq')
        assert np.isfinite(sums).all() and (sums[0] > 0 or flow == 'kida')     # (the Kida field vanishes on a 2^3 box)
        # without the two output fields, and once more: the same bits
        assert np.array_equal(d.ke(gpu_v), sums)
        assert np.array_equal(d.ke(gpu_v, out=(g_vsq, g_wsq)), sums)
    finally:
        d.release()


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('size', SHAPES[:3], ids=lambda s: 'x'.join(map(str, s)))
def test_ke_enstrophy_leaves_out_excluded_nodes(backend, size, precision):
    dtype = DTYPE[precision]
    v = _random_fields(size, dtype, 5)[1]
    rng = np.random.RandomState(3)
    unused = rng.random_sample(tuple(reversed(size))) < 0.2
    unused[0, 0, 0] = True
    d = Device(backend, size, precision, node_map=True)
    try:
        gpu_v = [d.field(c)[1] for c in v]
        gpu_map = d.map(unused)
        h_vsq, g_vsq = d.field(fill=np.nan)
        h_wsq, g_wsq = d.field(fill=np.nan)
        sums = d.ke(gpu_v, gpu_map, out=(g_vsq, g_wsq))
        want_vsq, want_wsq = tw.ke_fields(v, excluded=unused)      # neighbours differentiate across the unused nodes
        assert np.array_equal(d.real(d.fetch(h_vsq, g_vsq)), want_vsq)
        assert np.array_equal(d.real(d.fetch(h_wsq, g_wsq)), want_wsq)
        assert np.all(d.real(h_vsq)[unused] == 0) and np.all(d.real(h_wsq)[unused] == 0)
        _within(sums[0], want_vsq, 'sum v_sq')
        _within(sums[1], want_wsq, 'sum vort_sq')
        assert np.array_equal(d.ke(gpu_v, gpu_map), sums)
        # and without a map every node counts
        full = d.ke(gpu_v)
        _within(full[0], tw.ke_fields(v)[0], 'sum v_sq, no map')
        assert full[0] > sums[0]
    finally:
        d.release()


@pytest.mark.parametrize('precision', ['single', 'double'])
@pytest.mark.parametrize('size', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_profiles_kernel(backend, size, precision):
    dtype = DTYPE[precision]
    rho, v = _random_fields(size, dtype, 23)
    terms = tw.profile_terms(v, rho)
    d = Device(backend, size, precision)
    ring = 3
    try:
        gpu_v = [d.field(c)[1] for c in v]
        gpu_rho = d.field(rho)[1]
        for axis in range(3):
            n = size[axis]
            ref, bound = tw.profiles(terms, axis)
            ws = backend.stats_workspace(d.module, hipabi.SLF_STATS_PROFILES_X + axis)
            out = np.full((22, ring, n), -7.0)
            gpu_out = backend.alloc_buf(like=out)
            d._bufs += [ws, gpu_out]
            for snapshot in (1, 1, 2):                 # a non-zero offset; the same one again; the next one
                before = out.copy()
                backend.stats_profiles(d.module, axis, gpu_v, gpu_rho, ws, gpu_out, ring * n, snapshot * n, d.stream)
                d.stream.synchronize()
                backend.from_buf(gpu_out)
                got = out[:, snapshot, :]
                err = np.abs(got - ref)
                worst = np.unravel_index(np.argmax(err - bound), err.shape)
                print('axis %d snapshot %d: worst |diff| %.3e (bound %.3e) at statistic %s position %d'
                      % (axis, snapshot, err[worst], bound[worst], tw.PROFILE_KEYS[worst[0]], worst[1]))
                assert np.all(err <= bound)
                rest = np.ones(out.shape, dtype=bool)
                rest[:, snapshot, :] = False
                assert np.array_equal(out[rest], before[rest])       # nothing outside the snapshot is written
                if before[0, snapshot, 0] != -7.0:
                    assert np.array_equal(got, before[:, snapshot, :])   # a second call: the same bits
            assert np.all(out[:, 0, :] == -7.0)
    finally:
        d.release()


def test_argument_errors(backend):
    d = Device(backend, (8, 1, 4), 'single')
    try:
        gpu_v = [d.field(np.zeros((4, 1, 8)))[1] for _ in range(3)]
        with pytest.raises(backend.FatalError, match='extent of 1'):
            d.ke(gpu_v)
        with pytest.raises(backend.FatalError, match='NULL'):
            d.ke([gpu_v[0], 0, gpu_v[2]])
        with pytest.raises(backend.FatalError, match='together'):
            d.ke(gpu_v, out=(gpu_v[0], 0))
        ws = backend.stats_workspace(d.module, hipabi.SLF_STATS_PROFILES_Y)
        d._bufs.append(ws)
        with pytest.raises(backend.FatalError, match='axis'):
            backend.stats_profiles(d.module, 3, gpu_v, gpu_v[0], ws, d.gpu_sums, 8, 0, d.stream)
        with pytest.raises(backend.FatalError, match='NULL'):
            backend.stats_profiles(d.module, 0, gpu_v, 0, ws, d.gpu_sums, 8, 0, d.stream)
        with pytest.raises(backend.FatalError, match='out_stride'):
            backend.stats_profiles(d.module, 0, gpu_v, gpu_v[0], ws, d.gpu_sums, 8, 1, d.stream)
        m2 = backend.build(make_box_desc(sym.D2Q9, (16, 8)))
        with pytest.raises(backend.FatalError, match='3-D'):
            backend.stats_workspace(m2, hipabi.SLF_STATS_KE_ENSTROPHY)
        with pytest.raises(backend.FatalError, match='3-D'):
            backend.stats_ke_enstrophy(m2, 0, gpu_v, d.ke_ws, d.gpu_sums, 0, 0, d.stream)
    finally:
        d.release()


# ---- through the controller -----------------------------------------------------------------------------------------

def _host_v(sim):
    return np.array([np.array(c) for c in sim.v])


def _kida_sim(every=20):
    from examples.kida_vortex import KidaSim
    from sailfish.stats import KineticEnergyEnstrophyMixIn

    class Sim(KidaSim):
        """examples/kida_vortex.py's hook, with the host fields asked for at the iterations it samples (and a sample of
        the initial state)."""

        def before_main_loop(self, runner):
            KineticEnergyEnstrophyMixIn.before_main_loop(self, runner)
            self.samples = [(0, self.compute_ke_enstropy(runner), _host_v(self))]

        def after_step(self, runner):
            mod = self.iteration % every
            if mod == every - 1:
                self.need_fields_flag = True
                self.need_sync_flag = True           # ... and on the host
            elif mod == 0:
                self.samples.append((self.iteration, self.compute_ke_enstropy(runner), _host_v(self)))
    return Sim


def test_kida_box_through_the_controller():
    from tests.test_gpu_runner import run_gpu
    n, max_v = 24, 0.05
    ctrl = run_gpu(_kida_sim(), None, 3, dict(lat_nx=n, lat_ny=n, lat_nz=n, access_pattern='AA', precision='single',
                                              grid='D3Q19', visc=0.001375), 40)
    sim = ctrl.runners[0]._sim
    assert [s[0] for s in sim.samples] == [0, 20, 40]
    nodes = n ** 3
    for it, (ke, ens), v in sim.samples:
        assert v.dtype == np.float32
        v_sq, vort_sq = tw.ke_fields(v)
        for got, field, name in ((ke, v_sq, 'energy'), (ens, vort_sq, 'enstrophy')):
            ref, bound = tw.sum_and_bound(field, divisions=1, divisor=2.0 * nodes)
            print('iteration %d %s: %.12e, twin on the host fields %.12e, |diff| %.3e, bound %.3e'
                  % (it, name, got, ref, abs(got - ref), bound))
            assert isinstance(got, float) and abs(got - ref) <= bound
    # step 0: 3/8 max_v^2; the f32 field carries half an ulp per component, its square three, two additions one each
    e0 = 3.0 / 8.0 * max_v ** 2
    assert abs(sim.samples[0][1][0] - e0) <= 6 * 2.0 ** -24 * e0
    energies = [s[1][0] for s in sim.samples]
    assert energies[0] >= energies[1] >= energies[2] > 0
    # the per-node fields were stored: the host copy of the last step (taken before its sample) holds those of step 20
    assert np.array_equal(np.array(sim.v_sq), tw.ke_fields(sim.samples[1][2])[0])


def _channel_sim(ring):
    from sailfish.lb_base import LBForcedSim
    from sailfish.lb_single import LBFluidSim
    from sailfish.node_type import NTFullBBWall
    from sailfish.stats import ReynoldsStatsMixIn
    from sailfish.subdomain import Subdomain3D

    class Channel(Subdomain3D):
        def boundary_conditions(self, hx, hy, hz):
            self.set_node((hy == 0) | (hy == self.gy - 1), NTFullBBWall)

        def initial_conditions(self, sim, hx, hy, hz):
            sim.rho[:] = 1.0
            sim.vx[:] = 0.02 * np.sin(2 * np.pi * (hz + 0.5) / self.gz) * np.sin(np.pi * (hy + 0.5) / self.gy)
            sim.vz[:] = 0.01 * np.cos(2 * np.pi * (hx + 0.5) / self.gx)

    class Sim(LBFluidSim, LBForcedSim, ReynoldsStatsMixIn):
        subdomain = Channel
        stat_buf_size = ring
        axis = 'y'

        @classmethod
        def update_defaults(cls, defaults):
            defaults.update({'periodic_x': True, 'periodic_z': True, 'grid': 'D3Q19'})

        def __init__(self, config):
            super(Sim, self).__init__(config)
            self.add_body_force((1e-5, 0.0, 0.0))
            self.results, self.host = [], []

        def before_main_loop(self, runner):
            self.prepare_reynolds_stats(runner, axis=self.axis)
            self.need_sync_flag = True

        def after_step(self, runner):
            self.need_sync_flag = True              # every step stores its fields, on the device and on the host
            self.host.append((self.iteration, _host_v(self), np.array(self.rho)))
            self.results.append(self.collect_reynolds_stats(runner))
    return Sim


@pytest.mark.parametrize('axis', ['x', 'y', 'z'])
def test_reynolds_stats_ring_through_the_controller(axis):
    from tests.test_gpu_runner import run_gpu
    size = dict(lat_nx=16, lat_ny=10, lat_nz=12)
    Sim = _channel_sim(3)
    Sim.axis = axis
    ctrl = run_gpu(Sim, None, 3, dict(size, access_pattern='AB', precision='single', visc=0.05), 4)
    sim = ctrl.runners[0]._sim
    assert [r is None for r in sim.results] == [True, True, False, True]
    stats = sim.results[2]
    n = size['lat_n' + axis]
    norm = 16 * 10 * 12 // n
    assert sorted(stats) == sorted(tw.PROFILE_KEYS + ('iters',)) and stats['iters'] == [1, 2, 3]
    for snapshot, (it, v, rho) in enumerate(sim.host[:3]):
        assert it == snapshot + 1
        ref, bound = tw.profiles(tw.profile_terms(v, rho), 'xyz'.index(axis))
        for k, key in enumerate(tw.PROFILE_KEYS):
            assert stats[key].shape == (3, n) and stats[key].dtype == np.float64
            want = ref[k] / norm
            tol = bound[k] / norm + np.abs(want) * tw.U
            assert np.all(np.abs(stats[key][snapshot] - want) <= tol), (key, snapshot)
    assert np.ptp(stats['ux_m1']) > 0 and np.all(stats['rho_m1'] > 0.9)
    # the fourth call started a new ring
    assert sim.stat_cnt == 1 and sim.snapshot_iters == [4]


def _split_sim():
    from examples.kida_vortex import KidaSim
    from sailfish.stats import KineticEnergyEnstrophyMixIn, ReynoldsStatsMixIn

    class Sim(KidaSim, ReynoldsStatsMixIn):
        stat_buf_size = 1

        def before_main_loop(self, runner):
            KineticEnergyEnstrophyMixIn.before_main_loop(self, runner)

        def after_step(self, runner):
            if self.iteration == self.config.max_iters - 1:
                self.need_sync_flag = True
            if self.iteration == self.config.max_iters:
                self.profiles = {}
                for axis in 'xyz':
                    self.prepare_reynolds_stats(runner, axis=axis)
                    self.profiles[axis] = self.collect_reynolds_stats(runner)
                    self.profiles[axis]['norm'] = self._reyn_normalizer
                self.sum_v_sq = self.compute_ke_enstropy(runner)[0] * 2.0 * runner._spec.num_nodes
    return Sim


def test_two_subdomains_along_x_add_up_to_the_undivided_run():
    from tests.test_gpu_runner import merged_gpu, run_gpu
    size = (16, 12, 10)
    cfg = dict(lat_nx=size[0], lat_ny=size[1], lat_nz=size[2], access_pattern='AA', precision='single', grid='D3Q19',
               visc=0.01)
    one = run_gpu(_split_sim(), None, 3, cfg, 6)
    two = run_gpu(_split_sim(), None, 3, dict(cfg, subdomains=2, conn_axis='x'), 6)
    assert len(one.runners) == 1 and len(two.runners) == 2
    fields = {}
    for what in ('rho', 'v0', 'v1', 'v2'):
        fields[what] = merged_gpu(one, what)
        assert np.array_equal(fields[what], merged_gpu(two, what)), what      # the same flow, bit for bit
    v = np.array([fields['v0'], fields['v1'], fields['v2']])
    terms = tw.profile_terms(v, fields['rho'])
    whole = one.runners[0]._sim
    parts = [r._sim for r in sorted(two.runners, key=lambda r: r._spec.location[0])]
    for axis in 'xyz':
        ref, bound = tw.profiles(terms, 'xyz'.index(axis))
        norm = whole.profiles[axis]['norm']
        for k, key in enumerate(tw.PROFILE_KEYS):
            want = ref[k] / norm
            tol = bound[k] / norm + np.abs(want) * tw.U              # the sum, then a division
            if axis == 'x':
                joined = np.concatenate([p.profiles[axis][key][0] for p in parts])
            else:
                # each part divided by its own number of nodes per position: undone, the parts added, divided again --
                # four roundings, of numbers no larger than the parts' magnitudes (which may cancel in the total)
                sums = [p.profiles[axis][key][0] * p.profiles[axis]['norm'] for p in parts]
                joined = sum(sums) / norm
                tol = tol + 4 * tw.U * (sum(np.abs(x) for x in sums) / norm + np.abs(want))
            assert np.all(np.abs(whole.profiles[axis][key][0] - want) <= tol), (axis, key)
            assert np.all(np.abs(joined - want) <= tol), (axis, key)
    ref, bound = tw.sum_and_bound(tw.ke_fields(v)[0])
    tol = bound + 3 * abs(ref) * tw.U           # a division and a multiplication per run, one addition of the parts
    assert abs(whole.sum_v_sq - ref) <= tol
    assert abs(sum(p.sum_v_sq for p in parts) - ref) <= tol
