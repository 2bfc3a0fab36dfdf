"""The library's default strip height of the pair sweep (two rows whatever the box; slf_pair.hip) against
single stepping (SLF_STEP_PAIRS=0) of the same box, bit for bit: SLF_PAIR_ROWS and the placement knobs unset, on boxes
whose ny is a multiple of 4 (where the default used to be four rows) and on boxes where it is not.  Four-row strips stay
covered by the cases of tests/test_gpu_pair_prefetch.py and tests/test_gpu_pair_xcd.py that set SLF_PAIR_ROWS=4.
Helpers and what is compared: tests/test_gpu_pair_prefetch.py."""
import pytest

from tests.test_gpu_pair_prefetch import backend, _make, _paired, _result, _same, _single_reference, _slab  # noqa: F401

pytestmark = pytest.mark.gpu

STEPS = (2, 3, 8)
KNOBS = ('SLF_PAIR_XCD_LOG2', 'SLF_PAIR_MARCH')


def _run(backend, monkeypatch, shape, n, relax=True, zc=None, pf=None):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return _paired(backend, monkeypatch, shape, n, relax, ty=None, zc=zc, pf=pf)


# (shape, planes per chunk, relaxation): two strips that are each other's only neighbours, one wave, one plane; four
# strips and chunk seams; two waves and a ragged last chunk, with and without relaxation (a value staged or filed from
# the wrong row shows exactly); three waves and an odd strip-pair count; the full-width row with a chunk longer than the
# box; 32 strips, an active XCD map; 24 strips, the shift falls back to 0
CASES = [((64, 4, 1), 1, True), ((64, 8, 2), 1, True), ((128, 8, 5), 2, True), ((128, 8, 5), 2, False),
         ((192, 12, 7), 3, True), ((512, 8, 3), 8, True), ((64, 64, 3), 1, True), ((64, 48, 2), 2, True)]
IDS = ['%dx%dx%d-zc%d%s' % (s + (zc, '' if relax else '-norelax')) for s, zc, relax in CASES]


@pytest.mark.parametrize('n', STEPS)
@pytest.mark.parametrize('pf', [0, 1])
@pytest.mark.parametrize('shape,zc,relax', CASES, ids=IDS)
def test_default_rows_equal_single_stepping(backend, monkeypatch, shape, zc, relax, pf, n):
    ref = _single_reference(backend, monkeypatch, shape, n, relax)
    _same(_run(backend, monkeypatch, shape, n, relax, zc=zc, pf=pf), ref)


@pytest.mark.parametrize('shape,zc', [((192, 12, 7), 3), ((512, 8, 3), 8)], ids=['192x12x7', '512x8x3'])
def test_two_runs_in_one_process_are_equal(backend, monkeypatch, shape, zc):
    a = _run(backend, monkeypatch, shape, 8, zc=zc)
    b = _run(backend, monkeypatch, shape, 8, zc=zc)
    _same(b, a)


@pytest.mark.parametrize('shape', [(64, 64, 4), (64, 6, 4), (64, 2, 1)], ids=['ny64', 'ny6', 'ny2'])
def test_defaults_pair_and_are_correct(backend, monkeypatch, shape):
    """Every knob unset, planes per chunk included."""
    for n in (2, 5):
        ref = _single_reference(backend, monkeypatch, shape, n)
        _same(_run(backend, monkeypatch, shape, n), ref)
