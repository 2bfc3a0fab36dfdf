"""sailfish_amd/halo.py without a GPU: the one allocation path of the four halo schemes (order of the collective calls of
a zero-copy connector, one buffer or two per direction), the one face layout of the x-slab schemes, and the pack / unpack
kernels of the index-list scheme filed by step parity (CPU test backend, tests/_oracle_backend.py)."""
import ctypes
import os

import numpy as np
import pytest

from sailfish_amd import halo, xface
from sailfish_amd.subdomain_connection import Link
from tests import _host


class _Runner(object):
    float = np.float32


class RecordingConnector(object):
    """Stands in for connector.PeerConnector (zero_copy) / LocalConnector: hands out made-up addresses, logs every call."""

    def __init__(self, zero_copy, alloc=None):
        self.zero_copy = zero_copy
        self.calls = []
        self._next = 1 << 30
        self._alloc = alloc

    def _new(self, nelems):
        if self._alloc is not None:
            return self._alloc(max(1, nelems) * 4)
        self._next += 1 << 20
        return self._next

    def alloc_buffer(self, runner, nelems, dtype):
        self.calls.append(('alloc_buffer', nelems))
        return self._new(nelems)

    def alloc_recv(self, runner, kind, nid, parity, nelems, dtype):
        self.calls.append(('alloc_recv', kind, nid, parity, nelems))
        return self._new(nelems)

    def resolve(self, runner):
        self.calls.append(('resolve',))

    def send_addr(self, runner, kind, nid, parity):
        self.calls.append(('send_addr', kind, nid, parity))
        return self._new(1 << 16)


def _links(sizes):
    return dict((nid, Link(nid, n_send=ns, n_recv=nr)) for nid, (ns, nr) in sizes.items())


@pytest.mark.parametrize('separate', [False, True])
def test_zero_copy_allocation_resolves_once_whatever_the_links(separate):
    for kind in ('dist', 'macro'):
        conn = RecordingConnector(True)
        halo.allocate(conn, _Runner(), kind, {}, separate)
        assert conn.calls == [('resolve',)]           # a rank without links still takes part in the collective
        conn = RecordingConnector(True)
        links = _links({5: (10, 12), 2: (7, 7), 9: (0, 3)})
        halo.allocate(conn, _Runner(), kind, links, separate)
        want = [('alloc_recv', kind, nid, par, links[nid].n_recv) for nid in (2, 5, 9) for par in (0, 1)]
        want += [('resolve',)]
        want += [('send_addr', kind, nid, par) for nid in (2, 5, 9) for par in (0, 1)]
        assert conn.calls == want
        for link in links.values():                     # two receive sets of my own, two send sets in the neighbours' memory
            assert len(set(link.recv_bufs)) == 2 and len(set(link.send_bufs)) == 2


def test_copied_buffers_one_per_direction_for_index_lists_two_for_planes():
    conn = RecordingConnector(False)
    lists = _links({1: (10, 12), 3: (4, 0)})
    halo.allocate(conn, _Runner(), 'dist', lists, separate=False)
    assert conn.calls == [('alloc_buffer', 10), ('alloc_buffer', 12), ('alloc_buffer', 4), ('alloc_buffer', 0)]
    for link in lists.values():
        assert link.send_bufs[0] == link.send_bufs[1] and link.recv_bufs[0] == link.recv_bufs[1]
        assert link.send_bufs[0] != link.recv_bufs[0]
    conn = RecordingConnector(False)
    planes = _links({1: (10, 10)})
    halo.allocate(conn, _Runner(), 'dist', planes, separate=True)
    assert conn.calls == [('alloc_buffer', 10)] * 4
    link = planes[1]
    assert len(set(link.send_bufs + link.recv_bufs)) == 4


def _face_link(faces, send, recv):
    link = Link(0, faces=faces)
    link.send_bufs, link.recv_bufs = list(send), list(recv)
    return link


@pytest.mark.parametrize('faces', [[xface.LOW], [xface.HIGH], [xface.LOW, xface.HIGH]])
def test_face_layout_mine_low_high_the_neighbours_reversed(faces):
    n, isz = 100, 4
    send, recv = (1 << 20, 2 << 20), (3 << 20, 4 << 20)
    got = halo.face_layout(_face_link(faces, send, recv), n, isz)
    assert [(par, face) for par, face, _, _ in got] == [(par, face) for par in (0, 1) for face in faces]
    for par, face, s, r in got:
        k = faces.index(face)
        assert s - send[par] == k * n * isz                           # my send order: low, high -> offsets 0, n
        assert r - recv[par] == (len(faces) - 1 - k) * n * isz        # what I receive: the same, reversed


@pytest.mark.parametrize('faces', [[xface.LOW], [xface.HIGH], [xface.LOW, xface.HIGH]])
def test_face_layout_two_neighbours_agree(faces):
    """B's send buffer made A's receive buffer (controller.LocalGroup shares them so): what B sends through a face lies
    where A looks for what enters through the opposite face.  [LOW, HIGH]: a periodic run of two slabs."""
    n, isz = 64, 8
    opposite = sorted(1 - f for f in faces)               # B's faces towards A
    a = _face_link(faces, (1 << 20, 2 << 20), (3 << 20, 4 << 20))
    b = _face_link(opposite, a.recv_bufs, (5 << 20, 6 << 20))
    a_recv = dict(((par, face), r) for par, face, _, r in halo.face_layout(a, n, isz))
    b_send = dict(((par, face), s) for par, face, s, _ in halo.face_layout(b, n, isz))
    assert len(set(a_recv.values())) == 2 * len(faces)
    for par in (0, 1):
        for face in faces:
            assert b_send[(par, 1 - face)] == a_recv[(par, face)]


def _u64(addr, n):
    return np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctypes.c_uint64)), shape=(n,)).copy() if n else np.zeros(0, np.uint64)


@pytest.mark.parametrize('zero_copy', [False, True])
@pytest.mark.parametrize('pattern', ['AA', 'AB'])
def test_population_kernels_are_filed_by_the_parity_of_the_step_they_serve(pattern, zero_copy, tmp_path):
    """In place: parity 0 = the pull lists, parity 1 = the push lists, copy 0.  Two-copy: the push lists, the steps of
    parity p write copy 1 - p.  Lattice g of a link sits g * len(list) elements into the buffer of that parity."""
    from sailfish_amd import geo as geo_mod
    from sailfish_amd.controller import LBSimulationController
    sim_cls = _host.load_sim_class('ldc_3d', 'LDCSim')
    cfg = dict(lat_nx=14, lat_ny=10, lat_nz=8, visc=0.03, access_pattern=pattern, conn_axis='z', subdomains=2, max_iters=1,
               quiet=True, perf_stats_every=0, every=1, backends='tests._oracle_backend', output=str(tmp_path / 'o'),
               output_compress=False, gpus=[0])
    env = dict((k, os.environ.pop(k, None)) for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'))
    try:
        ctrl = LBSimulationController(sim_cls, geo_mod.EqualSubdomainsGeometry3D, default_config=cfg)
        ctrl.run(ignore_cmdline=True)
    finally:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
    assert len(ctrl.runners) == 2
    for r in ctrl.runners:
        h = r._halo
        if zero_copy:       # the same set-up again, buffers from a connector that keeps two sets per direction
            r._connector = RecordingConnector(True, alloc=lambda nbytes: r.backend.alloc_buf(size=nbytes))
            h = halo.IndexListHalo(r)
            assert [c[0] for c in r._connector.calls].count('resolve') == 1
        assert type(h) is halo.IndexListHalo and sorted(h.links) == [1 - r._spec.id] and not h.macro_links
        isz = 4
        for link in h.links.values():
            assert (link.send_bufs[0] != link.send_bufs[1]) == zero_copy and (link.recv_bufs[0] != link.recv_bufs[1]) == zero_copy
            assert link.n_send == max(len(link.push_send), len(link.pull_send)) > 0
            assert link.n_recv == max(len(link.push_recv), len(link.pull_recv)) > 0
            for par in (0, 1):
                mode, copy = (('pull', 0) if par == 0 else ('push', 0)) if pattern == 'AA' else ('push', 1 - par)
                for kernels, name, idx, bufs in ((link.packs, 'CollectSparseData', getattr(link, mode + '_send'), link.send_bufs),
                                                 (link.unpacks, 'DistributeSparseData', getattr(link, mode + '_recv'), link.recv_bufs)):
                    assert len(kernels[par]) == 1           # one lattice
                    k = kernels[par][0]
                    assert k.name == name
                    assert np.array_equal(_u64(k.args[0], len(idx)), idx)
                    assert k.args[1:] == [r.gpu_dist(0, copy), bufs[par] + 0 * len(idx) * isz, len(idx)]
        for par in (0, 1):
            assert h.messages('dist', par) == [(nid, l.send_bufs[par], l.n_send, l.recv_bufs[par], l.n_recv)
                                               for nid, l in sorted(h.links.items())]
        if not zero_copy:
            assert r.halo_messages('dist') == h.messages('dist', r._step_parity)
