"""Which strip a workgroup of the pair sweep takes (SLF_PAIR_XCD_LOG2) and the order in which phase A walks a strip's
rows (SLF_PAIR_MARCH; slf_pair.hip) against single stepping (SLF_STEP_PAIRS=0) of the same box, bit for
bit.  Both are placement for the L2 and nothing else: a strip map that is not one-to-one leaves strips unwritten or
written twice, a row staged or filed from the wrong place shows in the populations, and a misplaced wait reads stale
words sometimes -- hence the repeatability cases.

The shift the library picks is not visible through the C ABI; what the cases with an inactive map check is the result.
Helpers and what is compared: tests/test_gpu_pair_prefetch.py."""
import pytest

from tests.test_gpu_pair_prefetch import backend, _make, _paired, _result, _same, _single_reference, _slab  # noqa: F401

pytestmark = pytest.mark.gpu

STEPS = (2, 3, 8)
KNOBS = ('SLF_PAIR_XCD_LOG2', 'SLF_PAIR_MARCH')


def _run(backend, monkeypatch, shape, n, relax=True, ty=None, zc=None, pf=None, xcd=None, march=None):
    for name, val in zip(KNOBS, (xcd, march)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    return _paired(backend, monkeypatch, shape, n, relax, ty=ty, zc=zc, pf=pf)


# (rows per strip, shape, planes per chunk): 16 strips is the smallest active map, three chunks give the flat index a z
# part; 48 strips: the shift falls back from the limit to 1; 256 strips: the default limit of 5 in full; three waves per
# row and a ragged last chunk
MAPPED = [(2, (64, 32, 3), 1), (4, (64, 64, 3), 1), (2, (64, 96, 2), 2), (2, (64, 512, 2), 2), (4, (192, 64, 5), 2)]


@pytest.mark.parametrize('n', STEPS)
@pytest.mark.parametrize('pf', [0, 1])
@pytest.mark.parametrize('march', [0, 1])
@pytest.mark.parametrize('ty,shape,zc', MAPPED, ids=['%dx%dx%d-ty%d-zc%d' % (s + (ty, zc)) for ty, s, zc in MAPPED])
def test_mapped_strips_equal_single_stepping(backend, monkeypatch, ty, shape, zc, march, pf, n):
    assert (shape[1] // ty) % 16 == 0
    ref = _single_reference(backend, monkeypatch, shape, n)
    _same(_run(backend, monkeypatch, shape, n, ty=ty, zc=zc, pf=pf, march=march), ref)


@pytest.mark.parametrize('n', STEPS)
@pytest.mark.parametrize('pf', [0, 1])
@pytest.mark.parametrize('shape,ty,xcd', [((64, 24, 3), 2, None), ((64, 64, 3), 4, 0)], ids=['12-strips', 'switched-off'])
def test_inactive_map_equals_single_stepping(backend, monkeypatch, shape, ty, xcd, pf, n):
    """12 strips are no multiple of 8: strips as they come; SLF_PAIR_XCD_LOG2=0 on a box whose strips would be mapped."""
    ref = _single_reference(backend, monkeypatch, shape, n)
    _same(_run(backend, monkeypatch, shape, n, ty=ty, zc=1, pf=pf, xcd=xcd), ref)


def _march_cases(ty):
    # (shape, planes per chunk, relaxation): one strip that is its own neighbour (every halo row a wrapped own row); two
    # strips; an odd strip count (two upward strips meet across the wrap); three waves and a ragged chunk; the full-width
    # stage; pure propagation (a row staged or filed from the wrong place shows exactly)
    return [((64, ty, 1), 1, True), ((64, 2 * ty, 2), 1, True), ((64, 3 * ty, 3), 2, True), ((192, 12, 7), 3, True),
            ((512, 8, 3), 8, True), ((128, 8, 5), 2, False)]


MARCH = [(xcd, pf, ty) + c for xcd in (None, 0) for pf in (0, 1) for ty in (2, 4) for c in _march_cases(ty)]
MARCH_IDS = ['%s-pf%d-ty%d-%dx%dx%d-zc%d%s' % (('map' if xcd is None else 'nomap', pf, ty) + s + (zc, '' if relax else '-norelax'))
             for xcd, pf, ty, s, zc, relax in MARCH]


@pytest.mark.parametrize('n', STEPS)
@pytest.mark.parametrize('xcd,pf,ty,shape,zc,relax', MARCH, ids=MARCH_IDS)
def test_odd_strips_downwards_equal_single_stepping(backend, monkeypatch, xcd, pf, ty, shape, zc, relax, n):
    ref = _single_reference(backend, monkeypatch, shape, n, relax)
    _same(_run(backend, monkeypatch, shape, n, relax, ty=ty, zc=zc, pf=pf, xcd=xcd, march=1), ref)


@pytest.mark.parametrize('shape,zc', [((192, 12, 7), 3), ((512, 8, 3), 8)], ids=['192x12x7', '512x8x3'])
def test_two_runs_in_one_process_are_equal(backend, monkeypatch, shape, zc):
    """The shipped defaults (every knob of the kernel unset)."""
    a = _run(backend, monkeypatch, shape, 8, zc=zc)
    b = _run(backend, monkeypatch, shape, 8, zc=zc)
    _same(b, a)


@pytest.mark.parametrize('shape', [(64, 64, 4), (64, 6, 4)], ids=['ny64', 'ny6'])
def test_defaults_pair_and_are_correct(backend, monkeypatch, shape):
    """All knobs unset: 16 mapped four-row strips; ny = 6 pairs with three two-row strips as they come."""
    for n in (2, 5):
        ref = _single_reference(backend, monkeypatch, shape, n)
        _same(_run(backend, monkeypatch, shape, n), ref)


@pytest.mark.parametrize('name,value', [(KNOBS[0], v) for v in ('9', '-1', 'x')] + [(KNOBS[1], v) for v in ('2', 'x')])
def test_unsupported_value_is_refused_and_the_box_steps_singly(backend, monkeypatch, name, value):
    shape, n = (64, 8, 4), 4
    ref = _single_reference(backend, monkeypatch, shape, n)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(name, value)
    sim = _slab(backend, shape)
    assert sim.k_pair is None
    assert sim.pair_refused and sim.pair_refused.startswith('pair sweep:'), sim.pair_refused
    why = backend.set_kernel_pair(sim.k_sweep[0][0], 0, 0)
    assert why and why.startswith('pair sweep:') and name in why, why
    sim.init_synthetic(11)
    for _ in range(n):
        sim.step()
    assert sim.pair_launches == 0
    _same(_result(sim), ref)
