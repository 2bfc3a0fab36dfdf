"""Two time steps per launch of the two-copy periodic-box sweep (slf_pair.hip, C ABI slf_kernel_set_pair, deferred
stepping in sailfish_amd/box.py) against single stepping, bit for bit.

What is compared is the CURRENT copy (get_dist()) and the fields of a final step(save_macro=True).  The other copy is
not compared: under pairing it holds an older state by construction (a pair launch never writes the intermediate step)."""
import numpy as np
import pytest

from sailfish_amd import sym
from sailfish_amd.box import BoxSim, make_box_desc
from tests import _geometry as geo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def _slab(backend, shape, **kw):
    from sailfish_amd.slab import SlabSim
    return SlabSim(backend, sym.D3Q19, shape, rank=0, world=1, model='bgk', access_pattern='AB', visc=0.02, **kw)


def _result(sim):
    """(current populations, the same, rho and v after one more step with field output) over the real nodes -- with every
    axis wrapped in-sweep nothing reads or writes the ghost layers and the padding; releases the simulation."""
    dist = sim.real_view(sim.get_dist()).copy()
    assert sim.gpu_dist[sim.iteration & 1] == sim.gpu_dist[sim.current_dist_index()]
    sim.step(save_macro=True)
    rho, v = sim.fetch_fields()
    out = (dist, sim.real_view(sim.get_dist()).copy(), sim.real_view(rho).copy(), [sim.real_view(c).copy() for c in v])
    sim.release()
    return out


_singles = {}


def _single_reference(backend, monkeypatch, shape, n, seed=11):
    """Single stepping (SLF_STEP_PAIRS=0) of the same box: computed once per (shape, n), shared, never modified."""
    key = (shape, n, seed)
    if key not in _singles:
        monkeypatch.setenv('SLF_STEP_PAIRS', '0')
        sim = _slab(backend, shape)
        assert sim.k_pair is None
        sim.init_synthetic(seed)
        for _ in range(n):
            sim.step()
        _singles[key] = _result(sim)
        monkeypatch.delenv('SLF_STEP_PAIRS')
    return _singles[key]


def _same(got, ref):
    assert np.array_equal(got[0], ref[0]), 'populations after N steps'
    assert np.array_equal(got[1], ref[1]), 'populations after the step with field output'
    assert np.array_equal(got[2], ref[2]), 'rho'
    for a, b in zip(got[3], ref[3]):
        assert np.array_equal(a, b), 'velocity'


def _shapes(ty):
    # (shape, planes per chunk): one wave as its own x neighbour, the strip its own y neighbour, the plane its own z
    # neighbour; chunks of 2, 2, 1 (ragged last chunk, chunk seams); three waves (a ring that is no power of two); the
    # full-width row with a chunk longer than the box
    return [((64, ty, 1), 1), ((64, 2 * ty, 2), 1), ((128, 8, 5), 2), ((192, 12, 7), 3), ((512, 4, 3), 8)]


CASES = [(ty, shape, zc) for ty in (2, 4) for shape, zc in _shapes(ty)]


@pytest.mark.parametrize('n', [1, 2, 3, 7, 8])
@pytest.mark.parametrize('ty,shape,zc', CASES, ids=['ty%d-%dx%dx%d-zc%d' % ((t,) + s + (z,)) for t, s, z in CASES])
def test_pair_stepping_equals_single_stepping(backend, monkeypatch, ty, shape, zc, n):
    ref = _single_reference(backend, monkeypatch, shape, n)
    monkeypatch.setenv('SLF_PAIR_ROWS', str(ty))
    monkeypatch.setenv('SLF_PAIR_ZCHUNK', str(zc))
    sim = _slab(backend, shape)
    assert sim.k_pair is not None, sim.pair_refused
    sim.init_synthetic(11)
    for _ in range(n):
        sim.step()
    assert sim.pair_launches == n // 2          # n = 1 never launches the pair kernel; from n = 2 on it runs
    _same(_result(sim), ref)


def test_pair_stepping_without_relaxation(backend, monkeypatch):
    """relaxation_enabled off (propagation only): the slab driver cannot express it, the box driver can."""
    from tests._oracle_box import synthetic_fields
    size = (128, 8, 5)
    rho, v = synthetic_fields(size, 3)
    res = []
    for pairs in ('0', '1'):
        monkeypatch.setenv('SLF_STEP_PAIRS', pairs)
        monkeypatch.setenv('SLF_PAIR_ZCHUNK', '2')
        desc = make_box_desc(sym.D3Q19, size, precision='single', access_pattern='AB', visc=0.02, periodic_fused=[1, 1, 1],
                             relaxation_enabled=False)
        s = BoxSim(backend, desc, periodic=(True, True, True))
        assert (s.k_pair is not None) == (pairs == '1'), s.pair_refused
        s.set_fields(rho, v)
        s.initial_conditions()
        for _ in range(5):
            s.step()
        res.append(_result(s))
    _same(res[1], res[0])


SEQUENCES = {
    'step-sync-step-step-get': lambda s, d: (s.step(), s.sync(), s.step(), s.step(), s.get_dist()),
    'step-step_with_fields': lambda s, d: (s.step(), s.step(save_macro=True)),
    'step-set_dist': lambda s, d: (s.step(), s.set_dist(d)),
    'three-init-two': lambda s, d: ([s.step() for _ in range(3)], s.init_synthetic(5), s.step(), s.step()),
}


@pytest.mark.parametrize('name', sorted(SEQUENCES))
def test_interleavings(backend, monkeypatch, name):
    shape = (128, 8, 5)
    rng = np.random.RandomState(3)
    res = []
    for pairs in ('0', '1'):
        monkeypatch.setenv('SLF_STEP_PAIRS', pairs)
        monkeypatch.setenv('SLF_PAIR_ZCHUNK', '2')
        sim = _slab(backend, shape)
        assert (sim.k_pair is not None) == (pairs == '1')
        sim.init_synthetic(11)
        d = np.nan_to_num(sim.get_dist(), nan=0.0, posinf=0.0, neginf=0.0)      # (ghost layers, padding: never read)
        d = (d * (1.0 + 1e-3 * rng.rand(*d.shape))).astype(np.float32) if pairs == '0' else res[0][4]
        SEQUENCES[name](sim, d)
        it = sim.iteration
        got = sim.get_dist()
        # the array get_dist() read is gpu_dist[iteration & 1]
        raw = np.zeros((sim.Q, sim.stride), dtype=sim.dtype)
        backend.from_buf(sim.gpu_dist[it & 1], raw)
        assert np.array_equal(sim.real_view(raw[:, :sim.nodes].reshape(got.shape)), sim.real_view(got))
        res.append(_result(sim) + (d, it))
    assert res[0][5] == res[1][5]
    _same(res[1], res[0])


# case -> (what differs from the eligible box, what the library's reason names)
REFUSED = {
    'AA': (dict(access_pattern='AA'), 'two-copy'),
    'double': (dict(precision='double'), 'single precision'),
    'MRT': (dict(model='mrt'), 'BGK'),
    'node map': (dict(fluid_only=False, type_kind=geo.TYPE_KIND, nt_bits=geo.NT_BITS, node_params=[0.05, 0.0, 0.0],
                      periodic_fused=[0, 0, 0], periodic=(False, False, False), cavity=True), 'node map'),
    'body force': (dict(accel=[1e-5, 0.0, 0.0]), 'body force'),
    'nx = 96': (dict(size=(96, 8, 4)), 'multiple of 64'),
    'ny % rows': (dict(size=(64, 6, 4), rows=4), 'rows per strip'),
    'unwrapped axis': (dict(periodic_fused=[1, 0, 1]), 'wrapped'),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_step_singly_and_correctly(backend, monkeypatch, case):
    from tests._oracle_box import OracleBox, synthetic_fields
    kw = dict(precision='single', access_pattern='AB', visc=0.02, periodic_fused=[1, 1, 1])
    kw.update(REFUSED[case][0])
    size = kw.pop('size', (64, 8, 4))
    rows = kw.pop('rows', 2)
    periodic = kw.pop('periodic', (True, True, True))
    cavity = kw.pop('cavity', False)
    monkeypatch.setenv('SLF_PAIR_ROWS', str(rows))
    desc = make_box_desc(sym.D3Q19, size, **kw)
    nmap = geo.cavity_3d(desc) if cavity else None
    s = BoxSim(backend, desc, periodic=periodic, node_map=nmap)
    assert s.k_pair is None
    why = backend.set_kernel_pair(s.k_sweep[0][0], rows, 0)
    assert why and why.startswith('pair sweep:') and REFUSED[case][1] in why, why
    rho, v = synthetic_fields(size, 3, dtype=s.dtype)
    if cavity:
        rho, v = np.ones_like(rho), [np.zeros_like(c) for c in v]
    o = OracleBox(make_box_desc(sym.D3Q19, size, **kw), periodic=periodic, node_map=nmap)
    for sim in (s, o):
        sim.set_fields(rho, v)
        sim.initial_conditions()
        sim.run(4, save_last=False)
    assert s.pair_launches == 0
    got, ref = s.real_view(s.get_dist()), o.real_view(o.current_dist())
    fin = np.isfinite(ref)          # (the oracle marks what a wall node never receives)
    assert np.array_equal(got[fin], ref[fin])
    s.release()


def test_a_slab_with_a_halo_never_pairs():
    from sailfish_amd.backend_hip import HIPBackend
    from sailfish_amd.connector import RingExchanger

    class Opt(object):
        pass
    s = _slab(HIPBackend(Opt(), 0), (64, 8, 6), axis='z', force_halo=True, exchanger=RingExchanger(0, 1))
    assert s.k_pair is None
    s.init_synthetic(3)
    for _ in range(4):
        s.step()
    s.sync()
    assert s.pair_launches == 0
    s.release()
