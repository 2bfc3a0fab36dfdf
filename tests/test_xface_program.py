"""xface.program_chunks: the z-chunk loop of an x-connected subdomain's step (SubdomainRunner._program_xface,
SlabSim._program_xface) as pure host code, checked against ChunkPlan's own tables with a queue that only records."""
import itertools

import pytest

from sailfish_amd import xface
from tests._recording_queue import RecordingQueue, Stub


def test_step_kinds():
    assert xface.step_kinds(True, 0) == ('own', 'push') and xface.step_kinds(True, 6) == ('own', 'push')
    assert xface.step_kinds(True, 1) == ('push', 'own')
    assert xface.step_kinds(False, 0) == xface.step_kinds(False, 1) == ('push', 'push')


def run_program(plan, kind, prev_kind, nstreams, peer, every, exchanging=True, nkernels=2):
    n = len(plan.order)
    s0 = Stub('calc0')
    streams = [s0, Stub('calc1') if nstreams == 2 else s0]
    sh = Stub('data')
    events = tuple([Stub('%s%d' % (name, i)) for i in range(n)] for name in ('evc', 'evb', 'pevc', 'pevb'))
    kernels = [Stub('k%d' % i) for i in range(nkernels)]
    need = plan.peer_need(kind, prev_kind) if peer else plan.need[prev_kind]
    q = RecordingQueue()

    def after_chunk(pos):
        q.log.append(('after_chunk', sh, pos, None))
    xface.program_chunks(q, plan, 10, kernels, streams, sh, events, need, every, after_chunk if exchanging else None)
    return q.log, streams, sh, events, kernels, need


def index(log, entry, start=0, stop=None):
    """Position of the one occurrence of `entry` in log[start:stop]."""
    found = [i for i in range(start, len(log) if stop is None else stop) if log[i] == entry]
    assert len(found) == 1, (entry, found)
    return found[0]


CASES = list(itertools.product((0, 1), (1, 4), ((True, 0), (True, 1), (False, 0)), (1, 2), (False, True), (False, True)))


@pytest.mark.parametrize('wrap,nchunks,step,nstreams,peer,every', CASES)
def test_chunk_program_follows_the_plan(wrap, nchunks, step, nstreams, peer, every):
    plan = xface.ChunkPlan(40, wrap, nchunks)
    assert len(plan.chunks) == nchunks
    kind, prev_kind = xface.step_kinds(*step)
    log, streams, sh, (evc, evb, pevc, pevb), kernels, need = run_program(plan, kind, prev_kind, nstreams, peer, every)
    pos_of = dict((c, pos) for pos, c in enumerate(plan.order))
    assert len([e for e in log if e[0] == 'launch']) == len(plan.order) * len(kernels)
    end = 0
    for pos, c in enumerate(plan.order):
        st = streams[pos & 1]
        # every chunk once per kernel, its own region, on the stream of its position, in the plan's order
        at = [index(log, ('launch', st, k, plan.region(c, 10))) for k in kernels]
        assert at == sorted(at) and at[0] >= end
        first, last = at[0], at[-1]
        if need[c] >= 0:        # the transfer of the previous step that carries what it reads (or a later one: in order)
            assert any(e[0] == 'wait' and e[1] is st and e[2] in pevb[need[c]:] for e in log[:first])
        for c2 in plan.neighbours(c):
            if streams[pos_of[c2] & 1] is not st:
                assert ('wait', st, pevc[pos_of[c2]], None) in log[:first]
        nxt = len(log)
        if pos + 1 < len(plan.order):
            nxt = index(log, ('launch', streams[(pos + 1) & 1], kernels[0], plan.region(plan.order[pos + 1], 10)))
        if plan.exchanges_at(pos) or every or nstreams == 2:
            i = index(log, ('record', st, evc[pos], None), last + 1, nxt)
            i = index(log, ('wait', sh, evc[pos], None), i + 1, nxt)
            i = index(log, ('after_chunk', sh, pos, None), i + 1, nxt)
            end = index(log, ('record', sh, evb[pos], None), i + 1, nxt)
        else:                   # one stream, nothing travels, nobody waits: nothing is recorded for this chunk
            assert not [e for e in log if e[0] in ('record', 'after_chunk') and e[2] in (evc[pos], evb[pos], pos)]
            assert not [e for e in log if e[1] is sh and e[2] is evc[pos]]
            end = last + 1
    # nothing but launches, waits for the previous step, and this step's records / transfers
    for op, stream, what, _ in log:
        if op == 'wait' and stream is not sh:
            assert any(what is e for e in pevb + pevc)
        assert op in ('launch', 'wait', 'record', 'after_chunk')


@pytest.mark.parametrize('wrap,nchunks,nstreams,every', itertools.product((0, 1), (1, 4), (1, 2), (False, True)))
def test_without_an_exchange_nothing_touches_the_data_stream(wrap, nchunks, nstreams, every):
    """A same-process group moves the planes itself, on the chunk events: the loop records them and stops there."""
    plan = xface.ChunkPlan(40, wrap, nchunks)
    log, streams, sh, (evc, evb, _, _), kernels, _ = run_program(plan, 'push', 'push', nstreams, False, every, exchanging=False)
    assert not [e for e in log if e[1] is sh or e[2] in evb]
    for pos, c in enumerate(plan.order):
        last = index(log, ('launch', streams[pos & 1], kernels[-1], plan.region(c, 10)))
        recorded = [i for i, e in enumerate(log) if e == ('record', streams[pos & 1], evc[pos], None)]
        assert recorded == ([last + 1] if (plan.exchanges_at(pos) or every or nstreams == 2) else [])


# ---------------------------------------------------------------------------------------------------------------------
# The two callers: each names its own two conditions -- an event after every chunk, and who exchanges.  The methods
# run unbound on a stand-in that has just the attributes they read.

class Namespace(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def sparse_plan(monkeypatch):
    """Four chunks of which only the last two are followed by a transfer: the conditions show where nothing travels."""
    monkeypatch.setenv('SLF_XFACE_BATCHES', 'two')
    plan = xface.ChunkPlan(40, 0, 4)
    assert [plan.exchanges_at(pos) for pos in range(4)] == [False, False, True, True]
    return plan


def face_buffers(shared, plan):
    rows = [[Stub('buf%d%d' % (p, f)) for f in (0, 1)] for p in (0, 1)]
    return Namespace(send=rows, recv=rows, shared=shared, needs_clear=False, plane=7, nbytes=0)


def chunk_events(plan):
    return [[Stub('ev%d_%d' % (p, i)) for i in range(len(plan.order))] for p in (0, 1)]


@pytest.mark.parametrize('it', [0, 1])
@pytest.mark.parametrize('shared', [False, True])
def test_slab_records_every_chunk_and_signals_only_for_shared_planes(shared, it, monkeypatch):
    from sailfish_amd.slab import SlabSim
    plan = sparse_plan(monkeypatch)
    sweep, calc, halo = Stub('sweep'), Stub('calc'), Stub('halo')
    moved = []
    q = RecordingQueue()
    sim = Namespace(xface=face_buffers(shared, plan), chunks=plan, aa=True, calc_stream=calc, calc_stream2=Stub('calc2'),
                    module=Stub('module'), _ev_chunk=chunk_events(plan), _ev_batch=chunk_events(plan), time_halo=False,
                    halo_stream=halo, size=(64, 10, 40), _sweep_of=lambda it_, save: (sweep, 0, False),
                    _exchange=lambda q_, pieces: moved.append((len(q_.log), pieces)))
    SlabSim._program_xface(sim, q, it, False)
    kind = xface.step_kinds(True, it)[0]
    evc, evb = sim._ev_chunk[it & 1], sim._ev_batch[it & 1]
    want = []
    for pos in range(len(plan.order)):
        runs = plan.batches[kind][pos]
        recorded = ('record', calc, evc[pos], None) in q.log
        assert recorded == (shared or plan.exchanges_at(pos))        # shared planes: the neighbours count every chunk
        assert (('record', halo, evb[pos], None) in q.log) == recorded
        if recorded and (runs or shared):       # nothing to move, nobody to tell: no exchange
            want.append((index(q.log, ('wait', halo, evc[pos], None)) + 1, [(p0 * 7, (p1 - p0) * 7) for p0, p1 in runs]))
    assert moved == want and len(moved) == (4 if shared else 2)
    assert [e[2] for e in q.log if e[0] == 'launch'] == [sweep] * len(plan.order)


@pytest.mark.parametrize('it', [0, 1])
@pytest.mark.parametrize('shared,grouped', [(False, False), (True, False), (False, True), (True, True)])
def test_runner_records_every_chunk_only_on_its_own_and_a_group_exchanges_itself(shared, grouped, it, monkeypatch):
    from sailfish_amd.subdomain_runner import SubdomainRunner
    plan = sparse_plan(monkeypatch)
    calc, data, copied = Stub('calc'), Stub('data'), Stub('copied')
    kernels = [Stub('k0'), Stub('k1')]
    q = RecordingQueue()
    q.planned = True                            # (no timing bracket)
    sent = []
    connector = Namespace(enqueue_pieces=lambda q_, runner, pieces: sent.append((len(q_.log), pieces)))
    group = Namespace(single_calc_stream=False) if grouped else None
    r = Namespace(_profile=None, _xface=face_buffers(shared, plan), _xchunks=plan, config=Namespace(access_pattern='AA'),
                  _lat_size=(42, 12, 66), _calc_stream=calc, _bnd_stream=calc, module=Stub('module'), _data_stream=data,
                  _ev_chunk=chunk_events(plan), _ev_batch=chunk_events(plan), _connector=connector,
                  xface_pieces=lambda pos: ('pieces', pos), _neighbour_events=lambda g, name, par: [copied])
    SubdomainRunner._program_xface(r, q, it, kernels, group=group)
    evc, evb = r._ev_chunk[it & 1], r._ev_batch[it & 1]
    assert (('wait', calc, copied, None) in q.log) == grouped
    want = []
    for pos in range(len(plan.order)):
        recorded = ('record', calc, evc[pos], None) in q.log
        assert recorded == (plan.exchanges_at(pos) or (shared and not grouped))
        if grouped:                             # the group copies the planes, after the fronts of all its runners
            assert not [e for e in q.log if e[1] is data or e[2] is evb[pos]]
        elif recorded:
            want.append((index(q.log, ('wait', data, evc[pos], None)) + 1, ('pieces', pos)))
            assert q.log[want[-1][0]] == ('record', data, evb[pos], None)
    assert sent == want and len(sent) == (0 if grouped else 4 if shared else 2)
    assert len([e for e in q.log if e[0] == 'launch']) == len(kernels) * len(plan.order)
