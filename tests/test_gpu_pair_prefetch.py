"""The load paths of the pair sweep's phase A (SLF_PAIR_PREFETCH; slf_pair.hip) against single stepping,
bit for bit: 0 = the rows are loaded into registers and waited for, 1 = the next row is in flight to LDS (one
`global_load_lds_dword` per direction, per wave) while the current one collides.  The waits that order the staged words
are written by hand in the kernel; a missing or misplaced one does not fault, it reads stale words sometimes -- hence the
repeatability cases next to the comparisons.

What is compared is the CURRENT copy (get_dist()) and the fields of a final step(save_macro=True), as in
tests/test_gpu_pair.py."""
import numpy as np
import pytest

from sailfish_amd import sym
from sailfish_amd.box import BoxSim, make_box_desc

pytestmark = pytest.mark.gpu

SHIPPED = (1,)              # the values of SLF_PAIR_PREFETCH above 0 that the library serves
STEPS = (2, 3, 8)


@pytest.fixture(scope='module')
def backend():
    from sailfish_amd.backend_hip import HIPBackend

    class Opt(object):
        pass
    return HIPBackend(Opt(), 0)


def _slab(backend, shape):
    from sailfish_amd.slab import SlabSim
    return SlabSim(backend, sym.D3Q19, shape, rank=0, world=1, model='bgk', access_pattern='AB', visc=0.02)


def _box(backend, shape, **kw):
    """A BoxSim with synthetic fields (the slab driver cannot switch the relaxation off)."""
    from tests._oracle_box import synthetic_fields
    rho, v = synthetic_fields(shape, 3)
    desc = make_box_desc(sym.D3Q19, shape, precision='single', access_pattern='AB', visc=0.02, periodic_fused=[1, 1, 1], **kw)
    s = BoxSim(backend, desc, periodic=(True, True, True))
    s.set_fields(rho, v)
    s.initial_conditions()
    return s


def _make(backend, shape, relax):
    if relax:
        sim = _slab(backend, shape)
        sim.init_synthetic(11)
        return sim
    return _box(backend, shape, relaxation_enabled=False)


def _result(sim):
    dist = sim.real_view(sim.get_dist()).copy()
    sim.step(save_macro=True)
    rho, v = sim.fetch_fields()
    out = (dist, sim.real_view(sim.get_dist()).copy(), sim.real_view(rho).copy(), [sim.real_view(c).copy() for c in v])
    sim.release()
    return out


def _same(got, ref):
    assert np.array_equal(got[0], ref[0]), 'populations after N steps'
    assert np.array_equal(got[1], ref[1]), 'populations after the step with field output'
    assert np.array_equal(got[2], ref[2]), 'rho'
    for a, b in zip(got[3], ref[3]):
        assert np.array_equal(a, b), 'velocity'


_singles = {}


def _single_reference(backend, monkeypatch, shape, n, relax=True):
    """Single stepping (SLF_STEP_PAIRS=0) of the same box: computed once per case, shared, never modified."""
    key = (shape, n, relax)
    if key not in _singles:
        monkeypatch.setenv('SLF_STEP_PAIRS', '0')
        sim = _make(backend, shape, relax)
        assert sim.k_pair is None
        for _ in range(n):
            sim.step()
        _singles[key] = _result(sim)
        monkeypatch.delenv('SLF_STEP_PAIRS')
    return _singles[key]


def _paired(backend, monkeypatch, shape, n, relax=True, ty=None, zc=None, pf=None):
    for name, val in (('SLF_PAIR_ROWS', ty), ('SLF_PAIR_ZCHUNK', zc), ('SLF_PAIR_PREFETCH', pf)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    sim = _make(backend, shape, relax)
    assert sim.k_pair is not None, sim.pair_refused
    for _ in range(n):
        sim.step()
    assert sim.pair_launches == n // 2
    return _result(sim)


def _cases(ty):
    # (shape, planes per chunk, relaxation): one wave, the strip its own neighbour, one plane (every staged row is a wrapped
    # row and the stage is refilled with the same row); chunk seams on every plane; three waves (per-wave LDS bases that are
    # no power of two) and a ragged last chunk; the full-width row (the stage at its full size) with a chunk longer than
    # the box; pure propagation (a value staged from the wrong row or plane shows exactly)
    return [((64, ty, 1), 1, True), ((64, 2 * ty, 2), 1, True), ((192, 12, 7), 3, True), ((512, 4, 3), 8, True),
            ((128, 8, 5), 2, False)]


CASES = [(pf, ty) + c for pf in (0,) + SHIPPED for ty in (2, 4) for c in _cases(ty)]
IDS = ['pf%d-ty%d-%dx%dx%d-zc%d%s' % ((pf, ty) + s + (zc, '' if relax else '-norelax')) for pf, ty, s, zc, relax in CASES]


@pytest.mark.parametrize('n', STEPS)
@pytest.mark.parametrize('pf,ty,shape,zc,relax', CASES, ids=IDS)
def test_prefetch_equals_single_stepping(backend, monkeypatch, pf, ty, shape, zc, relax, n):
    ref = _single_reference(backend, monkeypatch, shape, n, relax)
    _same(_paired(backend, monkeypatch, shape, n, relax, ty=ty, zc=zc, pf=pf), ref)


@pytest.mark.parametrize('pf', SHIPPED)
@pytest.mark.parametrize('ty', [2, 4])
@pytest.mark.parametrize('shape,zc', [((192, 12, 7), 3), ((512, 4, 3), 8)], ids=['192x12x7', '512x4x3'])
def test_two_runs_in_one_process_are_equal(backend, monkeypatch, shape, zc, ty, pf):
    a = _paired(backend, monkeypatch, shape, 8, ty=ty, zc=zc, pf=pf)
    b = _paired(backend, monkeypatch, shape, 8, ty=ty, zc=zc, pf=pf)
    _same(b, a)


@pytest.mark.parametrize('shape', [(64, 8, 4), (64, 6, 4)], ids=['ny8', 'ny6'])
def test_defaults_pair_and_are_correct(backend, monkeypatch, shape):
    """Switch, rows and planes per chunk unset; ny = 6 is no multiple of 4 and can only pair with two-row strips."""
    for n in (2, 5):
        ref = _single_reference(backend, monkeypatch, shape, n)
        _same(_paired(backend, monkeypatch, shape, n), ref)


@pytest.mark.parametrize('value', ['7', '-1', 'x'])
def test_unsupported_value_is_refused_and_the_box_steps_singly(backend, monkeypatch, value):
    shape, n = (64, 8, 4), 4
    ref = _single_reference(backend, monkeypatch, shape, n)
    monkeypatch.setenv('SLF_PAIR_PREFETCH', value)
    sim = _slab(backend, shape)
    assert sim.k_pair is None
    assert sim.pair_refused and sim.pair_refused.startswith('pair sweep:'), sim.pair_refused
    why = backend.set_kernel_pair(sim.k_sweep[0][0], 0, 0)
    assert why and why.startswith('pair sweep:') and 'SLF_PAIR_PREFETCH' in why, why
    sim.init_synthetic(11)
    for _ in range(n):
        sim.step()
    assert sim.pair_launches == 0
    _same(_result(sim), ref)
